"""GPU tests of greedy acting through the layers: `FusedPolicy.greedy` (forward, state value, `srl_greedy_head`) against the
module in float64, the Stack-v2 layout through `policies.FusedOrientationGreedy`, and `Trainer(fused_eval=True).eval()`."""
import copy
import functools

import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

B = 20
U24 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _net():
  from stackrl_amd import nets
  return nets.DeepQSiamFCN(seed=4).cuda()


@functools.lru_cache(maxsize=None)
def _obs():
  g = torch.Generator(device='cuda').manual_seed(2)
  return (torch.randint(0, 256, (B, 128, 128, 2), generator=g, device='cuda', dtype=torch.uint8),
          torch.randint(0, 256, (B, 32, 32, 1), generator=g, device='cuda', dtype=torch.uint8))


def _xcorr64(x, w):
  """`layers.correlation` in float64 by the correlation theorem (no wrapped term at shifts up to H - h)."""
  H, h = x.shape[-1], w.shape[-1]
  c = torch.fft.irfft2(torch.fft.rfft2(x) * torch.fft.rfft2(w, s=(H, H)).conj(), s=(H, H)).sum(1, keepdim=True)
  return c[..., :H - h + 1, :H - h + 1]


@functools.lru_cache(maxsize=None)
def _reference():
  """The module's advantages in float64 on the host, once for all tests; left unchanged by them."""
  ref = copy.deepcopy(_net()).double().cpu()
  xm, xo = (t.cpu() for t in _obs())
  with torch.no_grad():
    x, _ = ref.left(xm.permute(0, 3, 1, 2).double() / 255.0)
    w, _ = ref.right(xo.permute(0, 3, 1, 2).double() / 255.0)
    return ref.pos(_xcorr64(x, w)).flatten(1).cuda()


@pytest.mark.parametrize('autocast', [None, torch.bfloat16], ids=['fp32-class', 'bf16'])
def test_fused_greedy_against_the_module(autocast):
  from stackrl_amd import qops
  net, x, adv64 = _net(), _obs(), _reference()
  pol = qops.FusedPolicy(chunk=8, autocast=autocast, fast=True)
  a, st, q = pol.greedy(net, x, stats=True, values=True)
  assert a.shape == (B,) and q.shape == (B, net.n_actions) and st.shape == (B, 4) and st.dtype == torch.float64
  assert torch.equal(a, torch.argmax(q, dim=-1))
  assert torch.equal(st[:, 0], q.amax(-1).double()) and torch.equal(st[:, 1], q.amin(-1).double())
  # the exploring path's action at epsilon 0 sits on a maximum of the returned Q (not necessarily the same index: (a - m) + v
  # is monotone in a and may merge neighbours, which is why ties need a rule)
  draws = qops.FusedPolicy.draws(net, B, torch.Generator(device='cuda').manual_seed(1), 'cuda')
  act = qops.FusedPolicy(chunk=8, autocast=autocast, fast=True)(net, x, 0.0, None, draws=draws)
  print('exploring path at epsilon 0: {} of {} actions are the greedy path\'s'.format(int((act == a).sum()), B))
  assert torch.equal(q.gather(1, act[:, None])[:, 0], q.amax(-1))
  # centred Q against the float64 module's: fp32-class 2 x 2e-4 of the largest |advantage| (the criterion
  # tests/test_rollout_forward_gpu.py holds the advantages to, doubled: the centring subtracts a mean with the same bound);
  # bf16: 2e-2 of the advantage range
  cq = q.double() - q.double().mean(-1, keepdim=True)
  c64 = adv64 - adv64.mean(-1, keepdim=True)
  tol = 2 * 2e-4 * adv64.abs().amax(-1) if autocast is None else 2e-2 * (adv64.amax(-1) - adv64.amin(-1))
  err = (cq - c64).abs().amax(-1)
  print('centred Q: largest error / tolerance {:.3g}'.format(float((err / tol).max())))
  assert bool((err <= tol).all())
  # the state value
  ff = pol._ff
  _, _, x0 = ff.features(x, bottom=True)
  assert x0.shape == (B, 8, 8, 256) and x0.is_contiguous() and x0.dtype == (torch.float32 if autocast is None else torch.bfloat16)
  v = pol.state_value(net, x0)
  d1, d2 = net.value[0], net.value[2]
  Bn, P, C, U = B, 64, 256, d1.out_features
  gam = (P + C + U + 4) * U24
  xd = x0.double().reshape(Bn, P, C)
  W1, b1, W2, b2 = (t.detach().double() for t in (d1.weight, d1.bias, d2.weight, d2.bias))
  pooled = xd.mean(1)
  e_pool = gam * xd.abs().mean(1)
  hid = (pooled @ W1.t() + b1).clamp(min=0)
  e_hid = gam * (pooled.abs() @ W1.abs().t() + b1.abs()) + e_pool @ W1.abs().t()
  want = hid @ W2[0] + b2[0]
  e_v = gam * (hid @ W2[0].abs() + b2[0].abs()) + e_hid @ W2[0].abs()
  with torch.no_grad():
    assert torch.allclose(want, copy.deepcopy(net.value).double()(pooled)[:, 0], rtol=1e-12, atol=1e-12)   # the layers written out are net.value's
  errv = (v.double() - want).abs()
  print('state value: largest error / bound {:.3g}'.format(float((errv / e_v).max())))
  assert bool((errv <= e_v).all())
  # and it is the value inside Q: q = (adv - m) + v, so the row mean of q is v up to the roundings of the head
  assert bool(((q.double().mean(-1) - v.double()).abs() <= 4 * 2.0 ** -23 * (q.abs().amax(-1).double() + v.abs().double())).all())


@pytest.mark.parametrize('autocast', [None, torch.bfloat16], ids=['fp32-class', 'bf16'])
def test_chunk_size_does_not_change_the_results(autocast):
  """20 samples in chunks of 8 and as one chunk (`chunk=32`): the same actions, Q and statistics, bit for bit.  Every chunk is
  evaluated as a multiple of eight samples and the cross-correlation is the row-product kernel at every batch size, so each
  sample goes through the same kernels with the same sums in the same order."""
  from stackrl_amd import qops
  net, x = _net(), _obs()
  a, st, q = qops.FusedPolicy(chunk=8, autocast=autocast, fast=True).greedy(net, x, stats=True, values=True)
  a2, st2, q2 = qops.FusedPolicy(chunk=32, autocast=autocast, fast=True).greedy(net, x, stats=True, values=True)
  print('chunk 32 against chunk 8: actions equal {}, Q equal {} (largest difference {:.3g}), stats equal {}'.format(
    torch.equal(a2, a), torch.equal(q2, q), float((q2 - q).abs().max()), torch.equal(st2, st)))
  assert torch.equal(a2, a) and torch.equal(q2, q) and torch.equal(st2, st)


@pytest.mark.parametrize('n_valid', [8, 5])
def test_stack_v2_layout_equals_the_expanded_observation(n_valid):
  """B = 4 envs of G = 8 object maps: the left U-Net and the value once per env (a batch of 4, evaluated as 8) against the
  expanded observation as 32 independent samples — both multiples of the routing batch, so every layer goes to the same
  kernel (tests/rollout_dispatch.py: the routing looks at the largest of 8, 4, 2, 1 that divides the batch), and the
  hand-written kernels work sample by sample: the same bytes."""
  from stackrl_amd import nets, qops
  from stackrl_amd.dqn import DQN
  from stackrl_amd.policies import FusedOrientationGreedy, expand_orientations
  import rollout_dispatch as D
  assert D.batch_class(8) == D.batch_class(32) == qops.FusedPolicy.ROUTING_BATCH
  Bn, G = 4, 8
  net = _net()
  g = torch.Generator(device='cuda').manual_seed(3)
  xm = torch.randint(0, 256, (Bn, 128, 128, 2), generator=g, device='cuda', dtype=torch.uint8)
  xo = torch.randint(0, 256, (Bn, G, 32, 32, 1), generator=g, device='cuda', dtype=torch.uint8)
  agent = DQN(net, collect_batch_size=Bn, replay_memory_size=2 * Bn, seed=9, policy_op=qops.FusedPolicy(chunk=32, fast=True), xcorr='bf16x3')
  a, q = FusedOrientationGreedy(agent, value=True)((xm, xo), n_valid=n_valid)
  A = net.n_actions
  assert a.shape == (Bn,) and q.shape == (Bn, G * A)
  ea, eq = qops.FusedPolicy(chunk=32, fast=True).greedy(net, expand_orientations((xm, xo)), values=True)
  assert eq.shape == (Bn * G, A)
  eq = eq.reshape(Bn, G, A).clone()
  eq[:, n_valid:] = -float('inf')
  eq = eq.reshape(Bn, G * A)
  assert torch.equal(q, eq) and torch.equal(a, torch.argmax(eq, dim=-1))
  assert torch.equal(FusedOrientationGreedy(agent)((xm, xo), n_valid=n_valid), a)
  # rows at or beyond n_valid hold garbage: nothing moves
  if n_valid < G:
    junk = xo.clone()
    junk[:, n_valid:] = torch.randint(0, 256, junk[:, n_valid:].shape, generator=g, device='cuda', dtype=torch.uint8)
    a2, q2 = FusedOrientationGreedy(agent, value=True)((xm, junk), n_valid=n_valid)
    assert torch.equal(a2, a) and torch.equal(q2, q)
  with pytest.raises(ValueError, match='n_valid'):
    FusedOrientationGreedy(agent)((xm, xo), n_valid=G + 1)


class _Recorder(object):
  """The agent seen through `greedy(stats=True)`, keeping every step's Q."""

  def __init__(self, agent):
    self.agent, self.values = agent, []

  def __getattr__(self, name):
    return getattr(self.agent, name)

  def greedy(self, inputs, stats=False, **kw):
    a, st, q = self.agent.greedy(inputs, stats=True, values=True, **kw)
    self.values.append(q)
    return (a, st) if stats else a


def test_fused_eval_streams_the_statistics(ref_pool):
  from stackrl_amd import env as envs, nets, qops
  from stackrl_amd.dqn import DQN
  from stackrl_amd.training import Trainer
  Bn, L = 64, 3

  def make():
    env = envs.make('Stack-v0', n_parallel=Bn, seed=5, pool=ref_pool, episode_length=L)
    net = nets.DeepQSiamFCN(env.observation_spec, seed=2).cuda()
    agent = DQN(net, collect_batch_size=Bn, replay_memory_size=2 * Bn, seed=9, policy_op=qops.FusedPolicy(chunk=32, fast=True),
                xcorr='bf16x3')
    return env, agent

  env, agent = make()
  A = agent.q_net.n_actions
  tr = Trainer(env, agent, eval_env=env, directory=None, eval_seed=7, fused_eval=True)
  # the working set of the loop itself, measured here: two steps of what `eval` does per step (the forward of one greedy call
  # and the env's step, with the previous step's observation still held), started from the state `eval` starts from
  def two_steps():
    env.seed(7)
    step = env.reset()
    step = step() if callable(step) else step
    for _ in range(2):
      a, _ = agent.greedy(step[0], stats=True)
      step = env.step(a)
      step = step() if callable(step) else step
  two_steps()                                              # first calls: packed weights, scratch
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  two_steps()
  torch.cuda.synchronize()
  working = torch.cuda.max_memory_allocated() - base
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  row = tr.eval()
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - base
  env.close()
  # an identically seeded second run, keeping every step's Q
  env2, agent2 = make()
  rec = _Recorder(agent2)
  row2 = Trainer(env2, rec, eval_env=env2, directory=None, eval_seed=7, fused_eval=True).eval()
  env2.close()
  values = torch.stack(rec.values).double()
  steps = values.shape[0]
  assert values.shape == (steps, Bn, A) and steps >= L
  want = (float(values.amax(dim=-1).mean()), float(values.mean()), float(values.std(unbiased=False)), float(values.min()), float(values.max()))
  print('fused eval row', row, 'from the stacked Q', want, 'steps', steps, 'peak', peak, 'working set', working)
  assert row[0] == 0 and row[1] == row2[1] and row == row2                 # the return: exactly
  for got, w in zip(row[2:], want):
    assert abs(got - w) <= 1e-9 * abs(w), (got, w)
  # no [steps, B, A] tensor: the plain path holds steps * B * A * 4 bytes at the end of the evaluation
  assert steps * Bn * A * 4 > 2 * Bn * A * 4
  assert peak <= working + 2 * Bn * A * 4, (peak, working)
