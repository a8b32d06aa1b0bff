"""CPU tests of the learner rows (N1, A1, A2, M1, T1) against the numpy/pure-Python oracle (oracle/dqn_oracle.py)
and closed forms, plus the world_size-2 `gloo` test of the gradient all-reduce."""
import math
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import dqn_oracle as O
from stackrl_amd import nets
from stackrl_amd.dqn import DQN, PolynomialDecay
from stackrl_amd.memory import ReplayMemory


def _small_net(seed=3):
  return nets.DeepQSiamFCN(input_spec=((16, 16, 2), (4, 4, 1)), left_filters=2, left_depth=2, pos_filters=2,
                           dueling_units=8, seed=seed)


def test_net_matches_reference_architecture():
  net = nets.DeepQSiamFCN(seed=1)
  parts = {k: sum(p.numel() for p in getattr(net, k).parameters()) for k in ['left', 'right', 'value', 'pos']}
  # ~2.13 M parameters (left 1.94 M, right 0.12 M, dueling 0.066 M, pos 2.5 K)
  assert parts == {'left': 1940944, 'right': 116736, 'value': 66049, 'pos': 2497}
  assert nets.count_parameters(net) == 2126226
  m = nets.forward_macs()
  assert abs(sum(m.values()) - 957e6) < 2e6 and abs(m['xcorr'] - 154e6) < 1e6     # 1.91 GFLOP forward
  assert net.n_actions == 9409 and net.out_hw == (97, 97)
  # same seed -> same weights (seed chain models.py:149-153), different seed -> different
  a, b, c = nets.DeepQSiamFCN(seed=1), nets.DeepQSiamFCN(seed=1), nets.DeepQSiamFCN(seed=2)
  assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
  assert not all(torch.equal(p, q) for p, q in zip(a.parameters(), c.parameters()))
  w = a.left.down[1][0].weight                       # he_normal: std = sqrt(2/fan_in), truncated at 2 sigma
  fan_in = w[0].numel()
  w = w.detach()
  assert abs(float(w.std()) - math.sqrt(2 / fan_in)) < 0.1 * math.sqrt(2 / fan_in)
  assert float(w.abs().max()) <= 2 * math.sqrt(2 / fan_in) / .8796 + 1e-6
  # transposed convolutions: Keras' Conv2DTranspose kernel is (kh, kw, out, in) and its fan_in is out * kh * kw
  up = nets.DeepQSiamFCN(seed=1).left.up[0]
  fan_in = up.out_channels * up.kernel_size[0] * up.kernel_size[1]
  assert abs(float(up.weight.detach().std()) - math.sqrt(2 / fan_in)) < 0.1 * math.sqrt(2 / fan_in)


def test_forward_shapes_scaling_and_dueling():
  net = _small_net()
  x = torch.randint(0, 256, (3, 16, 16, 2), dtype=torch.uint8)
  w = torch.randint(0, 256, (3, 4, 4, 1), dtype=torch.uint8)
  q = net((x, w))
  assert q.shape == (3, 13 * 13) and q.dtype == torch.float32
  # uint8 inputs are scaled by 1/255 (models.py:144-147): same result as float inputs already divided
  q2 = net((x.float() / 255, w.float() / 255))
  assert torch.allclose(q, q2, atol=1e-5)
  # dueling: Q = A - mean(A) + V  (models.py:188-192)
  xf, x0, wf = net.features((x, w))
  a = net.pos(nets.correlation_reference(xf, wf)).flatten(1)
  v = net.value(x0.mean(dim=(2, 3)))
  assert torch.allclose(q, a - a.mean(-1, keepdim=True) + v, atol=1e-5)
  assert torch.equal(q.argmax(-1), a.argmax(-1))       # what the fused policy head relies on


def test_correlation_against_loops():
  rng = np.random.RandomState(0)
  x = rng.normal(size=(2, 3, 9, 10)).astype(np.float32)
  w = rng.normal(size=(2, 3, 4, 5)).astype(np.float32)
  got = nets.correlation_reference(torch.from_numpy(x), torch.from_numpy(w)).numpy()
  np.testing.assert_allclose(got, O.xcorr(x, w), rtol=1e-5, atol=1e-5)


def test_polynomial_decay_matches_config_gin():
  eps = PolynomialDecay(1.0, 400000, .1, 1.0)          # config.gin:73-76
  assert eps(0) == 1.0 and abs(eps(200000) - 0.55) < 1e-12 and eps(400000) == eps(10 ** 7) == .1
  beta = PolynomialDecay(0.4, 400000, 1.0, 1.0)        # config.gin:78-81
  assert beta(0) == 0.4 and abs(beta(100000) - 0.55) < 1e-12 and beta(400000) == 1.0


@pytest.mark.parametrize('P,L,n,literal', [(1, 7, 1, False), (3, 5, 1, False), (3, 5, 1, True), (2, 9, 3, False)])
def test_replay_memory_against_restatement(P, L, n, literal):
  """Every add / set_terminal / update_priorities step leaves the same logits, flags and min/max trackers as the
  list-based restatement of memory.py, and the transition returned for each sampleable index is identical."""
  rng = np.random.RandomState(P * 100 + L)
  spec = (((P, 2, 2, 1), torch.uint8),)
  mem = ReplayMemory(spec, P * L, alpha=0.6, beta=0.5, n_steps=n, seed=0, reference_next_index=literal)
  mem.check = True
  ref = O.RefMemory(P, P * L, n_steps=n, literal_next_index=literal)
  assert mem.max_length == ref.L
  for t in range(4 * L):
    s = rng.randint(0, 255, size=(P, 2, 2, 1)).astype(np.uint8)
    r = rng.normal(size=P).astype(np.float32)
    term = rng.uniform(size=P) < (0.25 if n == 1 else 0.08)
    a = rng.randint(0, 50, size=P)
    # with nothing sampleable left when the slot holding the min logit is overwritten the reference asserts
    # ("No sampleable transition", memory.py:174-177): both sides must fail at the same step
    try:
      mem.add((torch.from_numpy(s),), torch.from_numpy(r), torch.from_numpy(term), torch.from_numpy(a))
      failed = False
    except FloatingPointError:
      failed = True
    try:
      ref.add(s, r, term, a)
      assert not failed
    except AssertionError:
      assert failed
      return
    if t % 7 == 6:
      mem.set_terminal(); ref.set_terminal()
    lg = mem._logits.numpy()
    assert np.array_equal(np.isfinite(lg), np.isfinite(np.array(ref.logits))), t
    fin = np.isfinite(lg)
    np.testing.assert_allclose(lg[fin], np.array(ref.logits)[fin], rtol=1e-6)
    assert np.array_equal(mem._terminal.numpy(), np.array(ref.terminal))
    assert mem._insert_index == ref.insert and len(mem) == int(fin.sum())
    idx = np.where(fin)[0]
    if len(idx) >= 2 and t % 3 == 2:
      pick = rng.choice(idx, size=min(3, len(idx)), replace=False)
      d = rng.uniform(0, 2, size=len(pick)).astype(np.float32)
      mem.update_priorities(torch.from_numpy(pick), torch.from_numpy(d))
      ref.update_priorities([int(i) for i in pick], d)
      assert int(mem._max_logit_index) == ref.max_idx and int(mem._min_logit_index) == ref.min_idx
      assert abs(float(mem._max_logit) - ref.max_logit) < 1e-6 and abs(float(mem._min_logit) - ref.min_logit) < 1e-6
    # index arithmetic (bit-exact) and gathered transition for every sampleable slot
    for i in idx:
      nxt = int(mem.next_indexes(torch.tensor(int(i)), n))
      assert nxt == ref.next_index(int(i), n)
      if not literal:
        assert nxt // L == int(i) // L                         # stays inside the env's partition
      st, ac, rew, nst, te = ref.transition(int(i))
      assert int(mem._actions[i]) == ac and bool(mem._terminal[nxt]) == te
      assert np.array_equal(mem._states[0][i].numpy(), st)
      if nst is not None:                                      # (the literal formula can point at a never-written slot)
        assert np.array_equal(mem._states[0][nxt].numpy(), nst)
  # sampling: without replacement, only sampleable slots, weights = exp(beta*alpha*(min_logit - logit))
  k = min(4, len(mem))
  if k:
    indexes, weights, (states, actions, rewards, next_states, terminal) = mem.sample(k, get_weights=True)
    ii = indexes.tolist()
    assert len(set(ii)) == k and all(math.isfinite(ref.logits[i]) for i in ii)
    for i, wgt in zip(ii, weights.tolist()):
      assert abs(wgt - ref.weight(i, 0.6, 0.5)) < 1e-5
    if n > 1:
      assert rewards.shape == (k, n)
      for row, i in zip(rewards.tolist(), ii):
        assert np.allclose(row, ref.transition(i)[2])
  with pytest.raises(FloatingPointError, match='Not enough elements'):       # memory.py:227-230
    mem.sample(len(mem) + 1)


def test_literal_next_index_leaves_partition():
  """The reference formula (memory.py:239-242) points into partition 0 for every other env: documented quirk."""
  mem = ReplayMemory((((4, 1, 1, 1), torch.uint8),), 40, reference_next_index=True)
  i = torch.tensor([3, 13, 29])
  assert mem.next_indexes(i, 1).tolist() == [4, 5, 2]          # (i+1)%10 + i//10
  assert ReplayMemory((((4, 1, 1, 1), torch.uint8),), 40).next_indexes(i, 1).tolist() == [4, 5, 2]   # and it is the default
  mem2 = ReplayMemory((((4, 1, 1, 1), torch.uint8),), 40, reference_next_index=False)       # the in-partition option
  assert mem2.next_indexes(i, 1).tolist() == [4, 14, 20]


@pytest.mark.parametrize('double,prioritized', [(True, True), (False, False)])
def test_dqn_update_math_against_numpy(double, prioritized):
  torch.manual_seed(0)
  net = _small_net()
  agent = DQN(net, learning_rate=1e-3, minibatch_size=6, replay_memory_size=4 * 12, discount_factor=.966667,
              collect_batch_size=4, exploration=0.5, prioritization=0.6 if prioritized else None,
              priority_bias_compensation=0.4 if prioritized else None, double=double, seed=5,
              target_update_period=3, adam_betas=(0.95, 0.95))
  rng = np.random.RandomState(1)
  for t in range(11):
    s = (torch.from_numpy(rng.randint(0, 256, (4, 16, 16, 2)).astype(np.uint8)),
         torch.from_numpy(rng.randint(0, 256, (4, 4, 4, 1)).astype(np.uint8)))
    agent.observe(s, torch.from_numpy(rng.normal(size=4).astype(np.float32)), torch.from_numpy(rng.uniform(size=4) < .2),
                  torch.from_numpy(rng.randint(0, net.n_actions, 4)))
  # make the target net differ from the online net
  with torch.no_grad():
    for p in agent._target_q_net.parameters():
      p.add_(0.01 * torch.randn_like(p))
  mem = agent._replay_memory
  state = mem._gen.get_state()
  if prioritized:
    idx, wts, (st, ac, rw, ns, te) = mem.sample(6, get_weights=True)
  else:
    st, ac, rw, ns, te = mem.sample(6); wts = None
  mem._gen.set_state(state)                      # train() will draw the same minibatch
  with torch.no_grad():
    q, qo, qt = agent._q_net(st), agent._q_net(ns), agent._target_q_net(ns)
  ref_loss, ref_mtd, ref_td = O.dqn_targets(q.numpy(), qo.numpy(), qt.numpy(), ac.numpy(), rw.numpy(), te.numpy(),
                                            .966667, double=double, weights=None if wts is None else wts.numpy())
  before = [p.detach().clone() for p in agent._params]
  loss, mtd = agent.train()
  assert abs(float(loss) - ref_loss) <= 1e-5 * max(1, abs(ref_loss)) and abs(float(mtd) - ref_mtd) <= 1e-5 * max(1, abs(ref_mtd))
  assert agent.iterations == 1 and any(not torch.equal(a, b) for a, b in zip(before, agent._params))
  if prioritized:                                # priorities <- log(|td| + 1e-3), memory.py:272
    np.testing.assert_allclose(mem._logits[idx].numpy(), np.log(ref_td + 1e-3), rtol=1e-4, atol=1e-5)
  # hard target sync every `target_update_period` iterations (dqn.py:478-484)
  agent.train()
  assert not all(torch.equal(a, b) for a, b in zip(agent._q_net.state_dict().values(), agent._target_q_net.state_dict().values()))
  agent.train()
  assert agent.iterations == 3
  assert all(torch.equal(a, b) for a, b in zip(agent._q_net.state_dict().values(), agent._target_q_net.state_dict().values()))


def test_policy_modes_and_argument_checks():
  net = _small_net()
  s = (torch.randint(0, 256, (5, 16, 16, 2), dtype=torch.uint8), torch.randint(0, 256, (5, 4, 4, 1), dtype=torch.uint8))
  a = DQN(net, exploration=0.0, collect_batch_size=5, replay_memory_size=50, seed=1)
  g, q = a.policy(s, values=True)
  assert torch.equal(g, q.argmax(-1)) and torch.equal(a.policy(s, exploration=True), g)      # eps = 0 -> greedy
  b = DQN(net, exploration=1.0, collect_batch_size=5, replay_memory_size=50, seed=1)
  acts = torch.stack([b.policy(s, exploration=True) for _ in range(20)])
  assert acts.min() >= 0 and acts.max() < net.n_actions and len(torch.unique(acts)) > 20     # eps = 1 -> uniform
  c = DQN(net, exploration_mode='boltzmann', exploration=1e-6, collect_batch_size=5, replay_memory_size=50, seed=1)
  assert torch.equal(c.policy(s, exploration=True), g)                                       # T -> 0 is greedy
  assert abs(DQN(net, exploration_mode=1, exploration=2.0, collect_batch_size=5, replay_memory_size=50).epsilon - math.exp(-.5)) < 1e-12
  with pytest.raises(ValueError, match=r'Must be in \[0,1\]'):
    DQN(net, exploration=1.5)                                                                # dqn.py:166-169
  with pytest.raises(ValueError, match='greater than 0'):
    DQN(net, exploration_mode='boltzmann', exploration=0.0)                                  # dqn.py:177-180
  with pytest.raises(TypeError):
    DQN('not a net')                                                                         # dqn.py:122-125
  sched = DQN(net, exploration=PolynomialDecay(1.0, 10, .1), collect_batch_size=5, replay_memory_size=50)
  assert sched.epsilon == 1.0


def _rank_main(rank, world, port, out):
  import torch.distributed as dist
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.manual_seed(0)
  net = _small_net(seed=7 + rank)                              # replicas built from DIFFERENT seeds: DQN broadcasts rank 0's
  agent = DQN(net, learning_rate=1e-2, minibatch_size=4, replay_memory_size=2 * 10, collect_batch_size=2, exploration=0.3,
              double=True, seed=100 + rank)                    # rank-local replay shard and sampling stream
  rng = np.random.RandomState(50 + rank)                       # rank-local env shard
  for t in range(9):
    s = (torch.from_numpy(rng.randint(0, 256, (2, 16, 16, 2)).astype(np.uint8)),
         torch.from_numpy(rng.randint(0, 256, (2, 4, 4, 1)).astype(np.uint8)))
    agent.observe(s, torch.from_numpy(rng.normal(size=2).astype(np.float32)), torch.zeros(2, dtype=torch.bool),
                  torch.from_numpy(rng.randint(0, net.n_actions, 2)))
  # local gradient of this rank's minibatch, computed without the collective
  st = agent._replay_memory._gen.get_state()
  states, actions, rewards, next_states, terminal = agent._replay_memory.sample(4)
  agent._replay_memory._gen.set_state(st)
  y = agent.td_targets(rewards, next_states, terminal)
  q = agent._q_net(states).gather(1, actions[:, None])[:, 0]
  agent._flat_grad.zero_()
  agent.loss_from_td((q - y).abs()).backward()
  local = agent._flat_grad.clone()
  gathered = [torch.zeros_like(local) for _ in range(world)]
  dist.all_gather(gathered, local)
  expect = torch.stack(gathered).mean(0)
  agent.train()                                                # all-reduce + identical Adam step on every replica
  flat = torch.cat([p.detach().flatten() for p in agent._params])
  allp = [torch.zeros_like(flat) for _ in range(world)]
  dist.all_gather(allp, flat)
  if rank == 0:
    torch.save({'grad_ok': bool(torch.allclose(agent._flat_grad, expect, atol=1e-7)),
                'replicas_equal': bool(torch.equal(allp[0], allp[1])),
                'grads_differ_across_ranks': bool(not torch.allclose(gathered[0], gathered[1]))}, out)
  dist.destroy_process_group()


def test_gradient_allreduce_world_size_2_gloo(tmp_path):
  import torch.multiprocessing as mp
  out = str(tmp_path / 'res.pt')
  port = 29000 + os.getpid() % 2000
  mp.spawn(_rank_main, args=(2, port, out), nprocs=2, join=True)
  res = torch.load(out)
  assert res == {'grad_ok': True, 'replicas_equal': True, 'grads_differ_across_ranks': True}


def test_env_shards_equal_one_batch(oracle_mod, ref_pool):
  """Multi-GPU sharding of the env path: rank g owns envs [g*B/G, (g+1)*B/G) with keys seed + offset + i
  (utils.py:433), no data exchange.  Two shards stepped separately give exactly the unsharded batch."""
  from stackrl_amd.config import StackConfig
  L = 4
  full = oracle_mod.OracleEnv(StackConfig(n_envs=6, episode_length=L), ref_pool, seed=21)
  lo = oracle_mod.OracleEnv(StackConfig(n_envs=3, episode_length=L, env_index_offset=0), ref_pool, seed=21)
  hi = oracle_mod.OracleEnv(StackConfig(n_envs=3, episode_length=L, env_index_offset=3), ref_pool, seed=21)
  (fm, fo), _, _ = full.reset()
  (lm, _), _, _ = lo.reset(); (hm, _), _, _ = hi.reset()
  assert np.array_equal(fm, np.concatenate([lm, hm]))
  for _ in range(L + 1):
    a = full.sample()
    assert np.array_equal(a, np.concatenate([lo.sample(), hi.sample()]))
    (fm, fo), fr, fd = full.step(a)
    (lm, lo_), lr, ld = lo.step(a[:3]); (hm, ho_), hr, hd = hi.step(a[3:])
    assert np.array_equal(fm, np.concatenate([lm, hm])) and np.array_equal(fo, np.concatenate([lo_, ho_]))
    assert np.array_equal(fr, np.concatenate([lr, hr])) and np.array_equal(fd, np.concatenate([ld, hd]))


def _bench_rank(rank, world, port, out):
  import torch.distributed as dist
  import bench
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  dist.init_process_group('gloo', rank=rank, world_size=world)
  dt, placed = bench.aggregate(1.0 + rank, 100 * (rank + 1), world, 'cpu')
  if rank == 0:
    torch.save({'dt': dt, 'placed': placed}, out)
  dist.destroy_process_group()


def test_bench_aggregation_world_size_2_gloo(tmp_path):
  """bench.py's N > 1 bookkeeping: value = placements of all ranks / max-over-ranks time."""
  import torch.multiprocessing as mp
  out = str(tmp_path / 'agg.pt')
  mp.spawn(_bench_rank, args=(2, 31000 + os.getpid() % 2000, out), nprocs=2, join=True)
  res = torch.load(out)
  assert res == {'dt': 2.0, 'placed': 300.0}


def test_bench_dump_outputs_float32_capped_fixed_sample(tmp_path, monkeypatch):
  """bench.py --dump-outputs: the last step's arrays as float32 .npy, every env while they fit the byte cap, else the same
  seeded sample of envs (in index order) on every run."""
  import bench
  B, H, h = 10, 8, 4
  om = torch.randint(0, 256, (B, H, H, 2), dtype=torch.uint8)
  oo = torch.randint(0, 256, (B, h, h, 1), dtype=torch.uint8)
  rw, dn = torch.randn(B), torch.rand(B) < 0.5
  bench.dump_env_outputs(str(tmp_path / 'all'), ((om, oo), rw, dn))
  got = {n: np.load(str(tmp_path / 'all' / (n + '.npy'))) for n in ('obs_map', 'obs_obj', 'reward', 'done')}
  assert all(a.dtype == np.float32 for a in got.values())
  assert np.array_equal(got['obs_map'], om.numpy()) and np.array_equal(got['obs_obj'], oo.numpy())
  assert np.array_equal(got['reward'], rw.numpy()) and np.array_equal(got['done'], dn.numpy())
  per_env = 4 * (H * H * 2 + h * h + 2)
  monkeypatch.setattr(bench, 'DUMP_BYTES', 3 * per_env + 1)
  for d in ('s1', 's2'):
    bench.dump_env_outputs(str(tmp_path / d), ((om, oo), rw, dn))
  s1, s2 = (np.load(str(tmp_path / d / 'obs_map.npy')) for d in ('s1', 's2'))
  assert s1.shape == (3, H, H, 2) and np.array_equal(s1, s2)
  idx = [i for i in range(B) if any(np.array_equal(om[i].numpy(), s) for s in s1)]
  assert len(idx) == 3 and np.array_equal(np.stack([om[i].numpy() for i in idx]), s1)


# ---------------------------------------------------------------------------- training loop, logs, checkpoints
class _ToyEnv(object):
  """The env interface `Training` uses (training.py:105, :267-275, :335-368) on CPU tensors: episodes of `L` steps,
  done on the L-th step, the step after a done is the reset step (reward 0, done False) like env.py:235-236."""

  def __init__(self, B, L, spec, seed=0):
    self.batch_size, self.L, self.spec = B, L, spec
    import collections
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

  def sample(self):
    return torch.randint(0, self.n_actions, (self.batch_size,), generator=self._g)

  def step(self, action):
    assert action.shape == (self.batch_size,) and int(action.max()) < self.n_actions
    self._t += 1
    if self._t % (self.L + 1) == 0:      # auto-reset call
      step = (self._obs(), torch.zeros(self.batch_size), torch.zeros(self.batch_size, dtype=torch.bool))
    else:
      done = torch.full((self.batch_size,), self._t % (self.L + 1) == self.L)
      step = (self._obs(), torch.rand(self.batch_size, generator=self._g), done)
    return lambda: step                  # non-blocking flavour: a callable, training.py:269-270


def _toy_agent(spec, B, seed):
  net = nets.DeepQSiamFCN(spec, left_filters=4, left_depth=2, pos_filters=4, dueling_units=8, seed=seed)
  return DQN(net, learning_rate=1e-3, minibatch_size=4, replay_memory_size=B * 8, discount_factor=.9,
             collect_batch_size=B, exploration=0.5, prioritization=0.6, priority_bias_compensation=0.5, double=True,
             seed=seed, target_update_period=3)


def test_metrics_follow_the_reference_semantics():
  from stackrl_amd import metrics
  m = metrics.AverageMetric(length=3)
  assert math.isnan(float(m.result)) and not m.full
  for v in (1., 2.):
    m += v
  assert float(m.result) == 1.5 and not m.full                     # partial buffer: sum / count (metrics.py:101-104)
  m += 6.; m += 10.                                                # wraps: [10, 2, 6]
  assert m.full and float(m.result) == 6.0 and m > 5 and m <= 6
  r = metrics.AverageReward(batch_size=3, length=2)
  r += (None, torch.tensor([1., 2., 3.]), torch.tensor([False, False, False]))
  r += (None, torch.tensor([1., 1., 1.]), torch.tensor([True, False, True]))   # returns 2 and 4 enter in env order
  assert r.full and float(r.result) == 3.0
  r += (None, torch.tensor([5., 1., 1.]), torch.tensor([True, True, False]))    # 5 then 4 replace them
  assert float(r.result) == 4.5
  r.reset()
  assert not r.full and float(r._episode_reward[2]) == 1.0                       # ongoing episodes are kept (metrics.py:168-173)
  r.reset(full=True)
  assert float(r._episode_reward.abs().sum()) == 0.0
  t = metrics.Timer()
  assert t() is None
  with t:
    pass
  with t:
    pass
  assert t.n == 2 and t(reset=False) >= 0.0 and t() is not None and t() is None


def test_training_loop_writes_the_reference_file_formats_and_resumes(tmp_path):
  from stackrl_amd.training import Trainer
  spec = ((16, 16, 2), (4, 4, 1))
  B, L = 3, 4
  d = str(tmp_path / 'run')

  def make():
    agent = _toy_agent(spec, B, seed=3)
    return agent, Trainer(_ToyEnv(B, L, spec, seed=1), agent, eval_env=_ToyEnv(2, L, spec, seed=2), directory=d,
                          log_interval=2, eval_interval=4, checkpoint_interval=4, eval_seed=5,
                          train_reward_buffer_length=2, eval_reward_buffer_length=4, save_evaluated_policies=True)

  agent, tr = make()
  tr.initialize(num_steps=6)
  losses = tr.run(8)
  assert losses.shape == (8,) and agent.iterations == 8
  rows = open(os.path.join(d, 'train.csv')).read().strip().split('\n')
  assert rows[0] == 'Iter,Return,Loss,MeanError,CollectTime,TrainTime'          # training.py:495-497
  assert [int(r.split(',')[0]) for r in rows[1:]] == [2, 4, 6, 8] and all(len(r.split(',')) == 6 for r in rows[1:])
  rows = open(os.path.join(d, 'eval.csv')).read().strip().split('\n')
  assert rows[0] == 'Iter,Return,Value,MeanValue,StdValue,MinValue,MaxValue'    # training.py:435-437
  assert [int(r.split(',')[0]) for r in rows[1:]] == [0, 4, 8]                  # initial evaluation + every 4
  vals = [float(x) for x in rows[-1].split(',')[1:]]
  assert vals[4] <= vals[2] <= vals[1] <= vals[5] and vals[3] >= 0                # min <= mean <= mean-of-max <= max
  assert os.path.isfile(os.path.join(d, 'saved_weights', '4', 'weights')) and os.path.isfile(os.path.join(d, 'saved_weights', '8', 'weights'))
  assert 'Running evaluation' in open(os.path.join(d, 'train.log')).read()
  assert os.path.isfile(os.path.join(d, 'checkpoint', 'ckpt.pt'))
  # same evaluation seed -> the evaluation env replays the same episodes: a second eval now gives the same row
  again = tr.eval()
  assert again[1:] == tuple(vals)
  # a fresh process: initialize() restores agent, memory and the return metric instead of collecting
  agent2, tr2 = make()
  assert agent2.iterations == 0
  tr2.initialize()
  assert agent2.iterations == 8
  for p, q in zip(agent._q_net.parameters(), agent2._q_net.parameters()):
    assert torch.equal(p, q)
  for p, q in zip(agent._target_q_net.parameters(), agent2._target_q_net.parameters()):
    assert torch.equal(p, q)
  assert torch.equal(agent._replay_memory._actions, agent2._replay_memory._actions)
  assert torch.equal(agent._replay_memory._logits, agent2._replay_memory._logits)
  assert float(tr2._reward.result) == float(tr._reward.result)
  # and continues: the next update draws the same minibatch and lands on the same weights in both
  la, _ = agent.train(); lb, _ = agent2.train()
  assert float(la) == float(lb)


def test_prefetch_restates_the_staleness_of_the_reference_pipeline():
  """`agents.DQN.prefetch = 3` (config.gin:104; dqn.py:247-252): minibatches are sampled `prefetch` updates before they are
  used.  (i) On a memory that does not change, the FIFO hands out the generator's minibatches in order, none lost or
  repeated.  (ii) Transitions that become sampleable after update 0 cannot be in the minibatches of updates 1 .. prefetch
  (those were drawn before), and turn up afterwards; without prefetch they can be drawn at once."""
  def agent(prefetch):
    a = DQN(_small_net(seed=2), learning_rate=1e-3, minibatch_size=3, replay_memory_size=8, discount_factor=.9,
            collect_batch_size=1, exploration=0.5, prioritization=None, double=True, seed=9, prefetch=prefetch)
    rng = np.random.RandomState(0)
    obs = lambda: (torch.from_numpy(rng.randint(0, 256, (1, 16, 16, 2)).astype(np.uint8)),
                   torch.from_numpy(rng.randint(0, 256, (1, 4, 4, 1)).astype(np.uint8)))
    for t in range(4):                     # actions 0, 1, 2 are sampleable (the newest transition has no successor yet)
      a.observe(obs(), torch.tensor([0.0]), torch.zeros(1, dtype=torch.bool), torch.tensor([t]))
    return a, obs
  seqs = {}
  for k in (None, 3):                      # (i)
    a, _ = agent(k)
    seqs[k] = [sorted(a._next_minibatch()[2][1].tolist()) for _ in range(6)]
  assert seqs[None] == seqs[3] == [[0, 1, 2]] * 6
  for k in (None, 2):                      # (ii)
    a, obs = agent(k)
    used = []
    for u in range(8):
      if u == 1:                           # three more transitions: actions 3, 4, 5 become sampleable
        for t in (4, 5, 6, 7):
          a.observe(obs(), torch.tensor([0.0]), torch.zeros(1, dtype=torch.bool), torch.tensor([t]))
      used.append(set(a._next_minibatch()[2][1].tolist()))
    old = {0, 1, 2}
    assert used[0] <= old
    if k:
      assert all(used[u] <= old for u in range(1, 1 + k)), used       # drawn before the new transitions existed
      assert any(not (used[u] <= old) for u in range(1 + k, 8)), used
    else:
      assert any(not (used[u] <= old) for u in range(1, 8)), used


def test_resume_continues_the_uninterrupted_run_with_prefetched_minibatches():
  """`DQN.state_dict` carries the minibatches already drawn and waiting (`dataset.prefetch`, dqn.py:247-252): an agent restored
  from it trains on the very minibatches the uninterrupted run trains on — same losses, same weights, bit for bit."""
  spec = ((16, 16, 2), (4, 4, 1))
  B = 3

  def make(seed):
    net = nets.DeepQSiamFCN(spec, left_filters=4, left_depth=2, pos_filters=4, dueling_units=8, seed=seed)
    return DQN(net, learning_rate=1e-3, minibatch_size=4, replay_memory_size=B * 8, discount_factor=.9, collect_batch_size=B,
               exploration=0.5, prioritization=0.6, priority_bias_compensation=0.5, double=True, seed=seed,
               target_update_period=3, prefetch=2)
  g = torch.Generator().manual_seed(0)
  a = make(3)
  for t in range(8):
    obs = (torch.randint(0, 256, (B, 16, 16, 2), generator=g, dtype=torch.uint8), torch.randint(0, 256, (B, 4, 4, 1), generator=g, dtype=torch.uint8))
    a.observe(obs, torch.rand(B, generator=g), torch.zeros(B, dtype=torch.bool), torch.randint(0, 169, (B,), generator=g))
  for _ in range(3):
    a.train()
  d = a.state_dict()
  assert 'prefetched' in d and len(d['prefetched']) == 2
  import copy
  d = copy.deepcopy(d)                # (the nets' state dicts are views of the live parameters)
  want = [float(a.train()[0]) for _ in range(4)]
  b = make(99)                        # other weights, other streams: everything comes from the state
  b.load_state_dict(d)
  got = [float(b.train()[0]) for _ in range(4)]
  assert got == want
  for p, q in zip(a._q_net.parameters(), b._q_net.parameters()):
    assert torch.equal(p, q)


def test_update_plan_against_the_table_of_modes():
  """`dqn.update_plan`: which stages of an update run together, on which stream, whether as a hipGraph, and which graph has
  the sampling generator registered — against the table written out by hand.  The stage order is always grad, fifo, reduce,
  apply; a segment ends at `reduce`, which is never inside a graph; with `early` (needs prefetch) `grad` ends its segment
  too, on the update stream; the draw is in `grad` without prefetch and in `fifo` with it.  Without graphs: the same stages
  in the same segments, none a graph, no generator registered."""
  from stackrl_amd.dqn import update_plan
  M, U = 'main', 'update'
  table = {  # (prefetch, world, early): [(stages, stream, graph, draws)]
    (0, 1, False): [(('grad', 'apply'), M, True, True)],
    (0, 1, True): [(('grad', 'apply'), M, True, True)],
    (0, 2, False): [(('grad',), M, True, True), (('reduce',), M, False, False), (('apply',), M, True, False)],
    (0, 2, True): [(('grad',), M, True, True), (('reduce',), M, False, False), (('apply',), M, True, False)],
    (2, 1, False): [(('grad', 'fifo', 'apply'), M, True, True)],
    (2, 1, True): [(('grad',), U, True, False), (('fifo', 'apply'), M, True, True)],
    (2, 2, False): [(('grad', 'fifo'), M, True, True), (('reduce',), M, False, False), (('apply',), M, True, False)],
    (2, 2, True): [(('grad',), U, True, False), (('fifo',), M, True, True), (('reduce',), M, False, False), (('apply',), M, True, False)],
  }
  for (prefetch, world, early), want in table.items():
    plan = update_plan(prefetch, world, early, True)
    assert [tuple(s) for s in plan] == want, (prefetch, world, early)
    stages = [name for s in plan for name in s.stages]
    assert stages == [n for n in ('grad', 'fifo', 'reduce', 'apply') if (n != 'fifo' or prefetch) and (n != 'reduce' or world > 1)]
    assert all(s.stages == ('reduce',) and not s.graph for s in plan if 'reduce' in s.stages)
    assert sum(s.draws for s in plan) == 1
    eager = update_plan(prefetch, world, early, False)
    assert [(s.stages, s.stream) for s in eager] == [(s.stages, s.stream) for s in plan]
    assert not any(s.graph or s.draws for s in eager)


def _ckpt_rank(rank, world, port, d, out):
  import torch.distributed as dist
  from stackrl_amd.training import Trainer
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  dist.init_process_group('gloo', rank=rank, world_size=world)
  spec = ((16, 16, 2), (4, 4, 1))
  B, L = 3, 4

  def make():
    agent = _toy_agent(spec, B, seed=3 + rank)                  # rank-local exploration / sampling streams
    return agent, Trainer(_ToyEnv(B, L, spec, seed=10 + rank), agent, directory=d, log_interval=2, checkpoint_interval=4,
                          train_reward_buffer_length=2)
  agent, tr = make()
  tr.initialize(num_steps=6)
  tr.run(4)                                                      # ends with a checkpoint at iteration 4
  agent2, tr2 = make()
  tr2.initialize()                                               # restores: shared file + this rank's own file
  same_mem = torch.equal(agent._replay_memory._actions, agent2._replay_memory._actions) and \
    all(torch.equal(a, b) for a, b in zip(agent._replay_memory._states, agent2._replay_memory._states))
  same_gen = torch.equal(agent._gen.get_state(), agent2._gen.get_state()) and \
    torch.equal(agent._replay_memory._gen.get_state(), agent2._replay_memory._gen.get_state())
  flat = torch.cat([p.detach().flatten() for p in agent2._params])
  allp = [torch.zeros_like(flat) for _ in range(world)]
  dist.all_gather(allp, flat)
  mem = agent2._replay_memory._states[0].flatten().float()
  allm = [torch.zeros_like(mem) for _ in range(world)]
  dist.all_gather(allm, mem)
  gen = agent2._replay_memory._gen.get_state().float()
  allg = [torch.zeros_like(gen) for _ in range(world)]
  dist.all_gather(allg, gen)
  torch.save({'iterations': agent2.iterations, 'own_memory_restored': bool(same_mem), 'own_generators_restored': bool(same_gen)}, out + str(rank))
  if rank == 0:
    torch.save({'weights_equal_across_ranks': bool(torch.equal(allp[0], allp[1])),
                'memories_differ_across_ranks': bool(not torch.equal(allm[0], allm[1])),
                'sampling_streams_differ_across_ranks': bool(not torch.equal(allg[0], allg[1])),
                'files': sorted(os.listdir(os.path.join(d, 'checkpoint')))}, out)
  dist.destroy_process_group()


def test_checkpoint_keeps_rank_local_state_per_rank_world_size_2_gloo(tmp_path):
  """One process per GPU: nets / optimiser / iteration counter are shared (rank 0 writes ckpt.pt), the replay shard, the
  exploration and sampling generators and the return metric are each rank's own (ckpt.rank<r>.pt).  After a resume every
  rank holds ITS memory and streams again — not copies of rank 0's, which would make the all-reduced gradient N copies of
  the same minibatch — and the replicas' weights are equal."""
  import torch.multiprocessing as mp
  d, out = str(tmp_path / 'run'), str(tmp_path / 'res.pt')
  mp.spawn(_ckpt_rank, args=(2, 27000 + os.getpid() % 2000, d, out), nprocs=2, join=True)
  res = torch.load(out)
  assert res == {'weights_equal_across_ranks': True, 'memories_differ_across_ranks': True,
                 'sampling_streams_differ_across_ranks': True, 'files': ['ckpt.pt', 'ckpt.rank0.pt', 'ckpt.rank1.pt']}
  for r in range(2):
    assert torch.load(out + str(r)) == {'iterations': 4, 'own_memory_restored': True, 'own_generators_restored': True}


def _failing_rank(rank, world, port, d, out):
  import datetime
  import torch.distributed as dist
  from stackrl_amd.training import Trainer
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
  spec = ((16, 16, 2), (4, 4, 1))
  B, L = 3, 4
  agent = _toy_agent(spec, B, seed=3 + rank)
  tr = Trainer(_ToyEnv(B, L, spec, seed=10 + rank), agent, directory=d, log_interval=2, checkpoint_interval=4,
               train_reward_buffer_length=2)
  tr.initialize(num_steps=6)
  if rank == 1:                        # this rank fails inside iteration 6, after the periodic checkpoint at 4
    real, calls = agent.train, {'n': 0}

    def train():
      calls['n'] += 1
      if calls['n'] == 6:
        raise ValueError('injected failure on rank 1')
      return real()
    agent.train = train
  err = None
  try:
    tr.run(8)
  except Exception as e:               # rank 1: the injected error; rank 0: its all-reduce loses the peer
    err = type(e).__name__
  ck = torch.load(os.path.join(d, 'checkpoint', 'ckpt.pt'), weights_only=False)
  torch.save({'error': err, 'checkpoint_iterations': int(ck['agent']['iterations'])}, out + str(rank))


def test_a_failing_rank_enters_no_collective_and_leaves_the_last_checkpoint_alone_world_size_2_gloo(tmp_path):
  """`run()` checkpoints in `finally` like the reference (training.py:405-408).  With several ranks the checkpoint ends in
  a barrier: a rank that raised inside the loop would enter it while its peer sits in the gradient all-reduce — mismatched
  collectives on one group — and rank 0 would later overwrite the good ckpt.pt.  Rank 1 fails in iteration 6 here: both
  ranks come back (no hang), and the checkpoint on disk is still the periodic one of iteration 4."""
  import torch.multiprocessing as mp
  d, out = str(tmp_path / 'run'), str(tmp_path / 'res.pt')
  ctx = mp.spawn(_failing_rank, args=(2, 25000 + os.getpid() % 2000, d, out), nprocs=2, join=False)
  t0 = time.time()
  while not ctx.join(timeout=5):
    assert time.time() - t0 < 240, 'a rank hangs in a collective'
  r0, r1 = torch.load(out + '0'), torch.load(out + '1')
  assert r1['error'] == 'ValueError' and r0['error'] is not None
  assert r0['checkpoint_iterations'] == 4 and r1['checkpoint_iterations'] == 4


def test_curriculum_moves_on_when_the_goal_return_is_reached(tmp_path):
  """training.py:120-158, :526-575 with toy envs: goal reached -> curriculum.csv row, next env, reset; after the last
  goal `stop_when_complete` ends the run; a new Trainer on the same directory skips the solved stages."""
  from stackrl_amd.training import Trainer
  spec = ((16, 16, 2), (4, 4, 1))
  B, L = 3, 4
  d = str(tmp_path / 'cur')
  made = []

  def stages(goals):
    for i, g in enumerate(goals):
      e = _ToyEnv(B, L, spec, seed=10 + i)
      made.append(e)
      yield e, g

  agent = _toy_agent(spec, B, seed=3)
  # toy rewards are U(0,1) per step -> episode returns around 2: goals 0.5 and 1.0 are reached at the first checks
  tr = Trainer(stages([0.5, 1.0]), agent, directory=d, log_interval=50, eval_interval=10 ** 9, checkpoint_interval=10 ** 9,
               train_reward_buffer_length=2, goal_check_interval=6)
  tr.initialize(num_steps=6)
  tr.run(40, stop_when_complete=True)
  rows = open(os.path.join(d, 'curriculum.csv')).read().strip().split('\n')
  assert rows[0] == 'EndIter,Goal' and [float(r.split(',')[1]) for r in rows[1:]] == [0.5, 1.0]   # training.py:531-536
  assert [int(r.split(',')[0]) for r in rows[1:]] == [6, 12] and agent.iterations == 12              # stopped when complete
  assert len(made) == 2 and tr._env is made[1] and tr._complete
  # resume: both goals are on file -> the curriculum is exhausted at construction
  made.clear()
  tr2 = Trainer(stages([0.5, 1.0]), _toy_agent(spec, B, seed=3), directory=d, goal_check_interval=6)
  assert tr2._complete and tr2._env is made[1]
  # a generator without goals is rejected (training.py:124-125)
  with pytest.raises(ValueError):
    Trainer(((e, None) for e in [_ToyEnv(B, L, spec)]), _toy_agent(spec, B, seed=3))


def test_env_path_names_follow_the_reference_rule():
  """`make(as_path=True)` (utils.py:89-127): first letter + three letters of the last word, or four letters."""
  from stackrl_amd import env as envs
  p = envs.make(as_path=True)
  assert p.startswith('StackEnv/elen30,urdf[5-9]?,odim0.125,uguiFalse') and p.endswith('factTrue,dtypuint8') and 'seed' not in p
  assert envs.make('Stack-v0', as_path=True, episode_length=8, seed=3).split('/')[1].startswith('elen8,')
  assert envs.make('Stack-v2', as_path=True) == 'TestStackEnv/ofreFalse,ofre3,kwarNone,urdf[5-9]?,rpar2,dtypuint8'


def _keras_conv2d_same(x, k, b):
  """Keras Conv2D(padding='same', activation='relu') on NHWC input with an HWIO kernel, written out."""
  B, H, W, C = x.shape
  kh, kw, _, O = k.shape
  xp = np.pad(x, ((0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2), (0, 0)))
  out = np.zeros((B, H, W, O), np.float64)
  for di in range(kh):
    for dj in range(kw):
      out += np.einsum('bhwc,co->bhwo', xp[:, di:di + H, dj:dj + W].astype(np.float64), k[di, dj].astype(np.float64))
  return np.maximum(out + b, 0)


def _keras_conv2d_transpose_2x2(x, k, b):
  """Keras Conv2DTranspose(kernel 2, strides 2, relu) on NHWC input, kernel (kh, kw, out, in)."""
  B, H, W, C = x.shape
  O = k.shape[2]
  out = np.zeros((B, 2 * H, 2 * W, O), np.float64)
  for di in range(2):
    for dj in range(2):
      out[:, di::2, dj::2] = np.einsum('bhwc,oc->bhwo', x.astype(np.float64), k[di, dj].astype(np.float64))
  return np.maximum(out + b, 0)


def test_keras_weight_import_layouts_and_names():
  import torch
  from stackrl_amd import nets, keras_weights as kw
  src = nets.DeepQSiamFCN(seed=1)
  w = kw.export_keras_weights(src)
  assert w['Left/convdw00/kernel:0'].shape == (3, 3, 2, 16) and w['Left/up3/kernel:0'].shape == (2, 2, 128, 256)
  assert w['Right/conv20/kernel:0'].shape == (3, 3, 32, 64) and w['dense/kernel:0'].shape == (256, 256)
  assert w['dense_1/kernel:0'].shape == (256, 1) and w['conv2d_2/kernel:0'].shape == (1, 1, 16, 1)
  assert len(w) == 2 * (22 + 12 + 2 + 3)      # Left 22 layers, Right 12, dueling 2, after the correlation 3
  # automatic names of a later model in the same process (dense_4, dense_5, conv2d_7 ...) resolve by order
  shifted = {}
  for k_, v in w.items():
    k_ = k_.replace('dense_1/', 'dense_5/').replace('dense/', 'dense_4/')
    for a, b_ in (('conv2d_2/', 'conv2d_9/'), ('conv2d_1/', 'conv2d_8/'), ('conv2d/', 'conv2d_7/')):
      if k_.startswith(a):
        k_ = k_.replace(a, b_); break
    shifted[k_] = v
  dst = nets.DeepQSiamFCN(seed=2)
  kw.load_keras_weights(dst, shifted)
  x = (torch.randint(0, 255, (2, 128, 128, 2), dtype=torch.uint8), torch.randint(0, 255, (2, 32, 32, 1), dtype=torch.uint8))
  with torch.no_grad():
    assert torch.equal(src(x), dst(x))
  # the layouts, against the Keras definitions written out in numpy
  rng = np.random.RandomState(0)
  xin = rng.rand(1, 8, 8, 2).astype(np.float32)
  ref = _keras_conv2d_same(xin, w['Left/convdw00/kernel:0'], w['Left/convdw00/bias:0'])
  got = torch.relu(dst.left.down[0][0](torch.from_numpy(xin).permute(0, 3, 1, 2))).permute(0, 2, 3, 1).detach().numpy()
  assert np.allclose(got, ref, atol=1e-5)
  xin = rng.rand(1, 4, 4, 256).astype(np.float32)
  ref = _keras_conv2d_transpose_2x2(xin, w['Left/up3/kernel:0'], w['Left/up3/bias:0'])
  got = torch.relu(dst.left.up[0](torch.from_numpy(xin).permute(0, 3, 1, 2))).permute(0, 2, 3, 1).detach().numpy()
  assert np.allclose(got, ref, atol=1e-4)
  xin = rng.rand(3, 256).astype(np.float32)
  ref = np.maximum(xin.astype(np.float64) @ w['dense/kernel:0'] + w['dense/bias:0'], 0)
  assert np.allclose(torch.relu(dst.value[0](torch.from_numpy(xin))).detach().numpy(), ref, atol=1e-4)
  # a checkpoint that does not fit is refused
  bad = dict(w); bad.pop('Right/up0/bias:0')
  with pytest.raises(KeyError):
    kw.load_keras_weights(nets.DeepQSiamFCN(seed=3), bad)
  bad = dict(w); bad['extra/kernel:0'] = np.zeros(3)
  with pytest.raises(ValueError):
    kw.load_keras_weights(nets.DeepQSiamFCN(seed=3), bad)


def test_bench_spawns_its_own_ranks_world_size_2_gloo():
  """`python bench.py --gpus 2` must start its two ranks itself (the driver calls it exactly so) and rank 0 must print
  one JSON line.  No GPU here: `--launch-only` runs spawn + rendezvous (gloo, 127.0.0.1) + barriers + the MAX / SUM
  aggregation and nothing else."""
  import json
  import subprocess
  import sys
  env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--launch-only', '--backend', 'gloo',
                      '--steps', '7', '--warmup', '2'], env=env, capture_output=True, text=True, timeout=300)
  assert p.returncode == 0, p.stderr[-2000:]
  lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1
  d = json.loads(lines[0])
  assert d['n_gpus'] == 2 and d['steps'] == 7 and d['warmup'] == 2 and d['value'] is None and d['launch_only']
  assert d['aggregate_check'] == {'max_dt': 1.5, 'sum_placed': 300.0}


def test_weight_packers_match_the_fragment_layouts_written_out():
  """`qops._pack` (cached flat gather index per layer shape) against the fragment layouts of include/stackrl_qnet.h
  written out with advanced indexing: 3 x 3 convolution (k = tap pairs at 16 input channels, tap x 32-channel blocks
  above), the implicit-GEMM order [cin / 32][tap][cout / 16][lane][8], the transposed convolution, and the hi / lo sets of
  the fp32-class kernels."""
  from stackrl_amd import qops
  lane = torch.arange(64)
  def conv(w):
    cout, cin = w.shape[:2]
    ks = torch.arange(5 if cin == 16 else 9 * (cin // 32))[:, None, None, None]
    mt = torch.arange(cout // 16)[None, :, None, None]; l = lane[None, None, :, None]; j = torch.arange(8)[None, None, None, :]
    k = 8 * (l >> 4) + j
    if cin == 16:
      tap, ci = 2 * ks + (k >> 4), k & 15
    else:
      m = cin // 32; tap, ci = ks // m + 0 * k, 32 * (ks % m) + k
    tc = tap.clamp(max=8)
    return (w.float()[16 * mt + (l & 15), ci, tc // 3, tc % 3] * (tap < 9)).to(torch.bfloat16).reshape(-1)
  def gemm(w):
    cout, cin = w.shape[:2]
    cb = torch.arange(cin // 32)[:, None, None, None, None]; tap = torch.arange(9)[None, :, None, None, None]
    mt = torch.arange(cout // 16)[None, None, :, None, None]; l = lane[None, None, None, :, None]; j = torch.arange(8)[None, None, None, None, :]
    return w.float()[16 * mt + (l & 15), 32 * cb + 8 * (l >> 4) + j, tap // 3, tap % 3].to(torch.bfloat16).reshape(-1)
  def convt(w):
    cin, cout = w.shape[:2]
    ks = torch.arange(cin // 32)[:, None, None, None]; mt = torch.arange(4 * cout // 16)[None, :, None, None]
    l = lane[None, None, :, None]; j = torch.arange(8)[None, None, None, :]
    m = 16 * mt + (l & 15); q, co = m // cout, m % cout
    return w.float()[32 * ks + 8 * (l >> 4) + j, co, q >> 1, q & 1].to(torch.bfloat16).reshape(-1)
  g = torch.Generator().manual_seed(0)
  split = lambda w: (w.to(torch.bfloat16).float(), w - w.to(torch.bfloat16).float())
  for cin, cout in ((16, 16), (16, 32), (32, 16), (64, 32)):
    w = torch.randn(cout, cin, 3, 3, generator=g)
    hi, lo = split(w)
    assert torch.equal(qops.pack_conv3x3_weights(w), conv(w))
    assert torch.equal(qops.pack_conv3x3_weights_x3(w), torch.cat([conv(hi), conv(lo)]))
  for cin, cout in ((32, 64), (256, 128)):
    w = torch.randn(cout, cin, 3, 3, generator=g)
    hi, lo = split(w)
    assert torch.equal(qops.pack_conv3x3_gemm_weights(w), gemm(w))
    assert torch.equal(qops.pack_conv3x3_gemm_weights(w, x3=True), torch.cat([gemm(hi), gemm(lo)]))
  for cin, cout in ((32, 16), (64, 32)):
    w = torch.randn(cin, cout, 2, 2, generator=g)
    hi, lo = split(w)
    assert torch.equal(qops.pack_convt2x2_weights(w), convt(w))
    assert torch.equal(qops.pack_convt2x2_weights_x3(w), torch.cat([convt(hi), convt(lo)]))
