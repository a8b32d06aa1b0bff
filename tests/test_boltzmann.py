"""CPU tests of Boltzmann exploration with per-sample random streams (include/stackrl_explore.h states the definition):
the torch restatement `stackrl_amd.dqn.philox4x32_10` / `boltzmann_noise`, `DQN.policy_draws` in Boltzmann mode, and the
plain path of `DQN.policy`, which keeps its `torch.rand` stream when no draws are handed in."""
import math

import pytest

torch = pytest.importorskip('torch')

from boltzmann_cases import FREQ_ADV, FREQ_T, check_frequencies, freq_keys
from stackrl_amd import nets
from stackrl_amd.dqn import DQN, boltzmann_noise, philox4x32_10


def _small_net(seed=3):
  return nets.DeepQSiamFCN(input_spec=((16, 16, 2), (4, 4, 1)), left_filters=2, left_depth=2, pos_filters=2,
                           dueling_units=8, seed=seed)


def _states(n, seed=0):
  g = torch.Generator().manual_seed(seed)
  return (torch.randint(0, 256, (n, 16, 16, 2), dtype=torch.uint8, generator=g),
          torch.randint(0, 256, (n, 4, 4, 1), dtype=torch.uint8, generator=g))


# Philox4x32-10 known answers (the Random123 test vectors)
PHILOX_KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def test_philox_known_answers():
  for counter, key, out in PHILOX_KAT:
    got = philox4x32_10(torch.tensor(counter, dtype=torch.int64), torch.tensor(key, dtype=torch.int64))
    assert got.dtype == torch.int64 and got.tolist() == list(out)
  # batched, with the key broadcast against the counters
  c = torch.tensor([k[0] for k in PHILOX_KAT[:2]], dtype=torch.int64)
  got = philox4x32_10(c, torch.tensor([[0, 0], [0xffffffff, 0xffffffff]], dtype=torch.int64))
  assert got.tolist() == [list(k[2]) for k in PHILOX_KAT[:2]]
  # the noise of action a is word a % 4 of the block with counter (a // 4, 0, 0, 0)
  keys = torch.tensor([[0xa4093822, 0x299f31d0], [7, 9]], dtype=torch.int64)
  z = boltzmann_noise(keys, 6, torch.float64)
  assert z.shape == (2, 6)
  for b in range(2):
    for a in range(6):
      x = int(philox4x32_10(torch.tensor([a // 4, 0, 0, 0], dtype=torch.int64), keys[b])[a % 4])
      u = ((x >> 9) + 0.5) * 2.0 ** -23
      assert abs(float(z[b, a]) + math.log(-math.log(u))) <= 1e-12


def test_uniform_range_is_open_and_exact_in_float32(monkeypatch):
  """x = 0 gives u = 2^-24 and x = 0xffffffff gives u = 1 - 2^-24; both are float32 numbers, and the noise is finite there."""
  from stackrl_amd import dqn
  lo, hi = 2.0 ** -24, 1.0 - 2.0 ** -24
  x = torch.tensor([0, 0xffffffff], dtype=torch.int64)
  for dtype in (torch.float32, torch.float64):
    u = dqn.boltzmann_uniform(x, dtype)
    assert u.dtype == dtype and u.tolist() == [lo, hi]
    assert u.float().double().tolist() == [lo, hi] and 0.0 < float(u.float()[0]) and float(u.float()[1]) < 1.0
  # the same two words through `boltzmann_noise` (the generator replaced by one that returns them)
  words = torch.tensor([0, 0xffffffff, 0x1ff, 0xfffffe00], dtype=torch.int64)        # the extremes and the other ends of their bins
  monkeypatch.setattr(dqn, 'philox4x32_10', lambda counter, key: words.expand(key.shape[0], counter.shape[1], 4))
  for dtype in (torch.float32, torch.float64):
    z = dqn.boltzmann_noise(torch.zeros((3, 2), dtype=torch.int64), 4, dtype)
    assert z.dtype == dtype and z.shape == (3, 4) and bool(torch.isfinite(z).all())
    ref = [-math.log(-math.log(lo)), -math.log(-math.log(hi))] * 2
    assert all(abs(float(g) - r) <= 1e-6 * abs(r) for g, r in zip(z[0], ref))


def test_groupwise_boltzmann_equals_whole_batch():
  net = _small_net()
  s = _states(5)
  agent = DQN(net, exploration_mode='boltzmann', exploration=0.7, collect_batch_size=5, replay_memory_size=50, seed=1)
  d = agent.policy_draws(5)
  assert isinstance(d, tuple) and len(d) == 1
  keys, = d
  assert keys.dtype == torch.int64 and keys.shape == (5, 2) and int(keys.min()) >= 0 and int(keys.max()) < 2 ** 32
  whole = agent.policy(s, exploration=True, draws=d)
  parts = [agent.policy(tuple(t[sl] for t in s), exploration=True, draws=tuple(x[sl] for x in d)) for sl in (slice(0, 2), slice(2, 5))]
  assert torch.equal(whole, torch.cat(parts))
  assert torch.equal(whole, agent.policy(s, exploration=True, draws=d))          # the draws are the whole randomness
  q = net(s)
  assert torch.equal(whole, torch.argmax(q / agent.exploration + boltzmann_noise(keys, q.shape[-1]), dim=-1))
  # a second set of draws continues the agent's generator
  assert not torch.equal(agent.policy_draws(5)[0], keys)


def test_boltzmann_without_draws_keeps_the_rand_stream():
  net = _small_net()
  s = _states(5)
  seed, e = 4, 0.7
  agent = DQN(net, exploration_mode='boltzmann', exploration=e, collect_batch_size=5, replay_memory_size=50, seed=seed)
  twin = DQN(net, exploration_mode='boltzmann', exploration=e, collect_batch_size=5, replay_memory_size=50, seed=seed)
  gen = torch.Generator().manual_seed(seed + 1)
  for _ in range(3):
    q = twin.policy(s, values=True)[1]
    ref = torch.argmax(q / e - torch.log(-torch.log(torch.rand(q.shape, generator=gen))), dim=-1)
    assert torch.equal(agent.policy(s, exploration=True), ref)


def test_frequencies_follow_the_softmax():
  adv = torch.tensor(FREQ_ADV, dtype=torch.float32)
  check_frequencies(torch.argmax(adv / FREQ_T + boltzmann_noise(freq_keys(), len(FREQ_ADV)), dim=-1))
