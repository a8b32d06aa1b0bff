"""GPU tests of Boltzmann exploration on the rollout path: the kernel `k_boltzmann_head` (csrc/qnet.hip) against the torch
restatement of its definition (include/stackrl_explore.h; `stackrl_amd.dqn.boltzmann_noise`), `FusedPolicy(mode='boltzmann')`
through `DQN.policy`, and group-wise collection in the training loop."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from boltzmann_cases import FREQ_ADV, FREQ_T, FREQ_N, check_frequencies, freq_keys

pytestmark = pytest.mark.gpu


def _keys(B, g):
  return torch.randint(0, 2 ** 32, (B, 2), dtype=torch.int64, generator=g, device='cuda')


@pytest.mark.parametrize('B,A', [(3, 1), (2, 3), (5, 4), (4, 5), (3, 1023), (3, 1024), (3, 1025), (2, 2401), (2, 9409)])
@pytest.mark.parametrize('T', [1e-6, 0.7, 50])
def test_kernel_against_the_restatement_in_float64(B, A, T):
  """The chosen action's float64 score is within four float32 roundings of the largest score's magnitude of the best one
  (the kernel's two logarithms and its divide are each good to about one rounding)."""
  from stackrl_amd import qops
  from stackrl_amd.dqn import boltzmann_noise
  g = torch.Generator(device='cuda').manual_seed(1000 * A + B)
  adv = 3 * torch.randn((B, A), generator=g, device='cuda')
  keys = _keys(B, g)
  got = qops.boltzmann_head(adv, keys, T)
  assert got.shape == (B,) and got.dtype == torch.int64 and int(got.min()) >= 0 and int(got.max()) < A
  q = adv.double() / float(np.float32(T))
  z = boltzmann_noise(keys, A, torch.float64)
  s64 = q + z
  margin = 4 * 2.0 ** -23 * (q.abs() + z.abs()).amax(-1)
  chosen = s64.gather(1, got[:, None])[:, 0]
  print('shortfall / margin:', ((s64.amax(-1) - chosen) / margin).tolist(), 'same as float64 arg-max:', (got == s64.argmax(-1)).tolist())
  assert bool((chosen >= s64.amax(-1) - margin).all())


@pytest.mark.parametrize('i,j', [(5, 6), (7, 7 + 1024), (9, 1030)])       # same quad; same thread, next stride; different threads
def test_ties_go_to_the_lowest_index(i, j):
  from stackrl_amd import qops
  g = torch.Generator(device='cuda').manual_seed(5)
  adv = torch.randn((4, 2049), generator=g, device='cuda')
  adv[:, i] = adv[:, j] = 1e30             # the noise is below the rounding of 1e30: the two scores are equal
  assert qops.boltzmann_head(adv, _keys(4, g), 1.0).tolist() == [i] * 4


def test_one_action():
  from stackrl_amd import qops
  g = torch.Generator(device='cuda').manual_seed(6)
  adv = torch.randn((7, 1), generator=g, device='cuda')
  assert qops.boltzmann_head(adv, _keys(7, g), 1.0).tolist() == [0] * 7     # 255 threads carry the sentinel and lose


def test_streams_belong_to_samples():
  from stackrl_amd import qops
  B, A = 64, 2401
  g = torch.Generator(device='cuda').manual_seed(7)
  adv = 3 * torch.randn((B, A), generator=g, device='cuda')
  keys = _keys(B, g)
  whole = qops.boltzmann_head(adv, keys, 0.7)
  s = torch.randperm(B, generator=g, device='cuda')
  assert torch.equal(qops.boltzmann_head(adv[s], keys[s], 0.7), whole[s])
  assert torch.equal(torch.cat([qops.boltzmann_head(adv[:32], keys[:32], 0.7), qops.boltzmann_head(adv[32:], keys[32:], 0.7)]), whole)
  # the key decides: one advantage row under two sets of keys
  row = adv[:1].expand(B, A).contiguous()
  a, b = qops.boltzmann_head(row, keys, 50.0), qops.boltzmann_head(row, _keys(B, g), 50.0)
  assert int((a != b).sum()) >= 60
  # and the rows of one call differ from one another: 64 nearly uniform draws from 2,401 actions collide 64 * 63 / 2 / 2401 =
  # 0.84 times on average; 8 collisions or more have a Poisson probability below 1e-6
  assert len(torch.unique(a)) > B - 8


def test_bad_arguments_raise_with_the_entry_points_message():
  from stackrl_amd import qops
  g = torch.Generator(device='cuda').manual_seed(8)
  adv = torch.randn((3, 5), generator=g, device='cuda')
  keys = _keys(3, g)
  for T in (0.0, -1.0, float('nan')):
    with pytest.raises(RuntimeError, match='srl_boltzmann_head: bad arguments'):
      qops.boltzmann_head(adv, keys, T)
  with pytest.raises(RuntimeError, match='srl_boltzmann_head: bad arguments'):
    qops.boltzmann_head(torch.empty((3, 0), device='cuda'), keys, 1.0)
  # keys that do not cover the batch never reach the kernel
  with pytest.raises(ValueError, match='keys must be'):
    qops.boltzmann_head(adv, keys[:2], 1.0)
  with pytest.raises(ValueError, match='keys must be'):
    qops.boltzmann_head(adv, keys.int(), 1.0)
  assert qops.boltzmann_head(adv, keys, 1.0).shape == (3,)


def test_kernel_frequencies_follow_the_softmax():
  from stackrl_amd import qops
  adv = torch.tensor(FREQ_ADV, dtype=torch.float32, device='cuda').expand(FREQ_N, len(FREQ_ADV)).contiguous()
  check_frequencies(qops.boltzmann_head(adv, freq_keys('cuda'), FREQ_T))


def test_fused_boltzmann_policy_grouped_and_whole():
  """`DQN.policy` on the fused rollout path in Boltzmann mode: the halves of a batch with the sliced draws take the actions
  of the whole batch (the rollout kernels work sample by sample from 256 samples per group), and a call without draws draws
  what `policy_draws` draws."""
  from stackrl_amd import nets, qops
  from stackrl_amd.dqn import DQN
  B = 512
  net = nets.DeepQSiamFCN(seed=4).cuda()
  g = torch.Generator(device='cuda').manual_seed(2)
  x = (torch.randint(0, 256, (B, 128, 128, 2), generator=g, device='cuda', dtype=torch.uint8),
       torch.randint(0, 256, (B, 32, 32, 1), generator=g, device='cuda', dtype=torch.uint8))

  def check(T):
    def agent():
      return DQN(net, exploration_mode='boltzmann', exploration=T, collect_batch_size=B, replay_memory_size=2 * B, seed=9,
                 policy_op=qops.FusedPolicy(chunk=256, fast=True), xcorr='bf16x3')
    a, twin = agent(), agent()
    d = twin.policy_draws(B)
    assert len(d) == 1 and d[0].shape == (B, 2) and d[0].dtype == torch.int64 and d[0].is_cuda
    whole = a.policy(x, exploration=True)                      # draws its own keys: the twin's
    assert torch.equal(whole, twin.policy(x, exploration=True, draws=d))
    assert int(whole.min()) >= 0 and int(whole.max()) < net.n_actions
    halves = [twin.policy(tuple(t[sl] for t in x), exploration=True, draws=tuple(k[sl] for k in d)) for sl in (slice(0, 256), slice(256, B))]
    assert torch.equal(torch.cat(halves), whole)
    return whole, twin
  _, twin = check(0.7)
  # On these observations the untrained net's advantage map has one peak far above 0.7: every sample takes it.  At a
  # temperature of the map's whole range no action's weight exceeds e times another's, so the 512 actions are spread over
  # the 9,409 and the equalities above compare the noise, not the peak.
  q = twin.policy(tuple(t[:8] for t in x), values=True)[1]
  whole, twin = check(float(q.max() - q.min()))
  assert len(torch.unique(whole)) > B // 2
  assert not torch.equal(twin.policy(x, exploration=True), whole)       # the generator's next keys: other actions


def test_groupwise_boltzmann_collection_equals_one_collect(ref_pool):
  """`test_groupwise_collection_equals_one_collect` of tests/test_learner_gpu.py with Boltzmann exploration under a scheduled
  temperature: the batch as two env groups takes the trajectories, replay contents, losses and weights of the one-handle loop,
  bit for bit."""
  from stackrl_amd import env as envs, nets, qops
  from stackrl_amd.dqn import DQN, PolynomialDecay
  from stackrl_amd.training import Trainer
  B, L = 512, 3
  runs = []
  for groups in (None, 2):
    env = envs.make('Stack-v0', n_parallel=B, seed=5, pool=ref_pool, episode_length=L, side_stream=True,
                    **({} if groups is None else dict(groups=groups)))
    assert getattr(env, 'groups', 1) == (groups or 1)
    net = nets.DeepQSiamFCN(env.observation_spec, seed=2).cuda()
    agent = DQN(net, learning_rate=6.25e-5, adam_betas=(0.95, 0.95), minibatch_size=8, replay_memory_size=B * 8,
                discount_factor=.966667, collect_batch_size=B, exploration_mode='boltzmann',
                exploration=PolynomialDecay(2.0, 1000, 0.1), prioritization=0.6,
                priority_bias_compensation=PolynomialDecay(0.4, 400000, 1.0), double=True, seed=9,
                policy_op=qops.FusedPolicy(chunk=256, fast=True), xcorr='bf16x3', prefetch=3)
    tr = Trainer(env, agent)
    tr.initialize(num_steps=2)
    losses = tr.run(2 * (L + 1) + 1)       # two episodes and a step: through the auto-reset call of every group
    mem = agent._replay_memory
    runs.append((losses.clone(), [p.detach().clone() for p in net.parameters()], mem._actions.clone(), mem._rewards.clone(),
                 mem._states[0].clone(), mem._states[1].clone(), float(tr.returns) if tr.returns is not None else None))
    env.close()
  a, b = runs
  assert torch.equal(a[2], b[2]), 'actions'
  assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]), 'stored transitions'
  assert torch.equal(a[0], b[0]), 'losses'
  for p, q in zip(a[1], b[1]):
    assert torch.equal(p, q)
  assert a[6] == b[6]
