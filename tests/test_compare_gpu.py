"""GPU tests of the policy-comparison kernel (csrc/compare.hip through `compare.MapStatistics`) against the numpy float64
restatement `compare.compare_reference`, and of `compare.run` on `VecStackEnv` end to end."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

# (P, B, A): one element; the scripted shape; around one sweep of 256 threads; eight policies at the product's 97 x 97 maps;
# more envs than one step of k_fold's loop is likely to get wrong
SHAPES = [(1, 1, 1), (2, 3, 81), (3, 2, 255), (3, 2, 256), (3, 2, 257), (8, 3, 9409), (5, 70, 81)]
IDS = ['{}x{}x{}'.format(*s) for s in SHAPES]
U53 = 2.0 ** -53


def _dtype(j):
  return torch.float64 if j % 2 else torch.float32       # odd policies hand in float64 maps (the baselines do)


@functools.lru_cache(maxsize=None)
def _maps(shape, kind):
  """P host tensors [B, A] and the restatement's (record, amax) of them: computed once, shared and left unchanged."""
  from stackrl_amd import compare
  P, B, A = shape
  g = torch.Generator().manual_seed(1000 * P + B + A)
  if kind == 'int':
    maps = [torch.randint(-8, 9, (B, A), generator=g).to(_dtype(j)) for j in range(P)]
  else:
    maps = [(torch.randn((B, A), generator=g) * (1 + j) + 0.25 * j).to(_dtype(j)) for j in range(P)]
  return maps, compare.compare_reference(maps)


def _device_record(shape, maps, steps=1):
  from stackrl_amd import compare
  P, B, A = shape
  st = compare.MapStatistics(P, A, 'cuda')
  amax = [st.step([m.cuda() for m in maps]) for _ in range(steps)]
  return st.result(), amax[-1].cpu().numpy()


def _sum_bounds(maps, P):
  """Per record entry 2 (n - 1) 2^-53 sum |terms|: the distance two summation orders of n terms can be apart (each within
  (n - 1) u sum |terms| of the exact sum, to first order; the terms themselves are exact: float32 values and their products)."""
  from stackrl_amd import compare
  x = np.stack([m.float().double().numpy() for m in maps])
  n = x.shape[1] * x.shape[2]
  terms = [np.abs(x[j]).sum() for j in range(P)] + [np.abs(x[i] * x[j]).sum() for i, j in compare.pair_index(P)]
  return 2 * (n - 1) * U53 * np.array(terms)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_integer_maps_give_the_restatements_record_bit_for_bit(shape):
  maps, (want, want_amax) = _maps(shape, 'int')
  got, amax = _device_record(shape, maps)
  assert np.array_equal(amax, want_amax)
  assert np.array_equal(got, want), np.nonzero(got != want)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_float_maps_sums_within_the_reordering_bound_and_flags_exact(shape):
  from stackrl_amd import compare
  P, B, A = shape
  maps, (want, want_amax) = _maps(shape, 'float')
  # on the CPU first: no value so near a threshold that the order of the threshold's own sums could move its flag (one
  # element is its own mean in any order, and sigma is 0: no flag either way)
  x = np.stack([m.float().double().numpy() for m in maps])
  mu = x.mean(-1, keepdims=True)
  thr2 = mu + x.std(-1, keepdims=True)
  if A > 1:
    for thr in (mu, thr2):
      assert np.all(np.abs(x - thr) > 1e-9 * np.maximum(1.0, np.abs(thr)))
  got, amax = _device_record(shape, maps)
  assert np.array_equal(amax, want_amax)
  n_sums = P + P * (P + 1) // 2
  assert got[0] == want[0] == B
  err = np.abs(got[1:1 + n_sums] - want[1:1 + n_sums])
  bound = _sum_bounds(maps, P)
  print('sums: largest error / bound', float((err / np.maximum(bound, 1e-300)).max()) if A > 1 else 0.0)
  assert np.all(err <= bound)
  assert np.array_equal(got[1 + n_sums:], want[1 + n_sums:])            # the counts
  if shape == (8, 3, 9409):                                             # a second identical run: the same bits
    again, _ = _device_record(shape, maps)
    assert again.tobytes() == got.tobytes()


def test_float64_inputs_are_rounded_to_float32():
  """1 + 2^-30 counts as 1: a float64 map is the float32 map it rounds to."""
  shape = (2, 3, 81)
  maps, (want, _) = _maps(shape, 'int')
  bumped = [m.double() + (2.0 ** -30) * (torch.arange(81) % 3 == j).double() * m.double().abs() for j, m in enumerate(maps)]
  assert all(not torch.equal(b, m.double()) and torch.equal(b.float(), m.float()) for b, m in zip(bumped, maps))
  ones = [torch.ones(3, 81, dtype=torch.float64) + 2.0 ** -30, torch.ones(3, 81)]
  got, amax = _device_record(shape, bumped)
  assert np.array_equal(got, want)
  got, amax = _device_record(shape, ones)
  assert np.array_equal(amax, np.ones((2, 3), np.float32))
  assert got[1] == got[2] == got[3] == got[4] == got[5] == 3 * 81 and not got[6:].any()     # s, S; no value above its mean


def test_edge_maps():
  from stackrl_amd import compare
  B, A = 2, 300
  g = torch.Generator().manual_seed(5)
  base = torch.randint(1, 9, (B, A), generator=g).float()
  nan = base.clone(); nan[0, 17] = float('nan')
  inf = base.clone().double(); inf[1, 299] = float('inf')
  maps = [torch.full((B, A), 3.0), base, base.clone().double(), nan, inf]
  P = len(maps)
  want, want_amax = compare.compare_reference(maps)
  got, amax = _device_record((P, B, A), maps)
  assert np.array_equal(amax, want_amax, equal_nan=True) and np.isnan(amax[3, 0]) and amax[4, 1] == np.inf
  assert np.array_equal(got, want, equal_nan=True)
  assert np.isnan(got).any() and np.isinf(got).any()
  with np.errstate(all='ignore'):
    m = compare.matrices(got, P, A)
  assert np.isnan(m['corrcoef'][0]).all()                   # a constant map: sigma = 0, d = 0
  assert m['corrcoef'][1, 2] == 1.0 and m['corrcoef'][1, 1] == 1.0 and m['overlap_mean'][1, 2] == 1.0 and m['overlap_std'][1, 2] == 1.0
  assert np.isnan(m['overlap_mean'][0, 0]) and m['overlap_mean'][0, 1] == 0.0      # the constant map flags nothing
  u = compare.unpack(got, P)
  # the NaN map flags nothing in env 0 (a NaN threshold): what is left is what the clean map flags in env 1
  clean = compare.unpack(compare.compare_reference([base[1:], base[1:]])[0], 2)
  assert u['I1'][3, 3] == clean['I1'][0, 0]


def test_steps_accumulate_onto_the_record():
  from stackrl_amd import compare
  shape = (2, 3, 81)
  P, B, A = shape
  g = torch.Generator().manual_seed(8)
  steps = [[torch.randint(-8, 9, (B, A), generator=g).to(_dtype(j)) for j in range(P)] for _ in range(3)]
  st = compare.MapStatistics(P, A, 'cuda')
  for maps in steps:
    st.step([m.cuda() for m in maps])
  want, _ = compare.compare_reference([torch.cat([s[j].double() for s in steps]) for j in range(P)])
  assert np.array_equal(st.result(), want) and want[0] == 9
  st.reset()
  assert not st.result().any()


def test_grouped_maps_take_the_chosen_row():
  from stackrl_amd import compare
  P, B, G, A = 3, 5, 4, 257
  g = torch.Generator().manual_seed(9)
  maps = [torch.randint(-8, 9, (B, G * A), generator=g).to(_dtype(j)) for j in range(P)]
  acts = [torch.randint(0, G * A, (B,), generator=g) for _ in range(P)]
  rows = [compare._chosen_rows(m, a, A) for m, a in zip(maps, acts)]
  want, want_amax = compare.compare_reference(rows)
  st = compare.MapStatistics(P, A, 'cuda')
  amax = st.step([m.cuda() for m in maps], [a.cuda() for a in acts])
  assert np.array_equal(amax.cpu().numpy(), want_amax) and np.array_equal(st.result(), want)
  cpu = compare.MapStatistics(P, A)
  cpu.step(maps, acts)
  assert np.array_equal(cpu.result(), want)


def test_refusals_launch_nothing():
  from stackrl_amd import compare
  lib = compare.load()
  P, B, A = 2, 3, 81
  R = compare.record_doubles(P)
  maps = [torch.ones(B, A, device='cuda') for _ in range(P)]
  amax = torch.full((P, B), 7.0, device='cuda')
  partial = torch.full((B, R), 7.0, dtype=torch.float64, device='cuda')
  record = torch.full((R,), 7.0, dtype=torch.float64, device='cuda')
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

  def step(P=P, A=A, ptrs=None, out=(amax, partial, record)):
    ptrs = [m.data_ptr() for m in maps] + [None] * 6 if ptrs is None else ptrs
    return lib.srl_compare_step(P, *ptrs[:8], 0, B, 1, A, None, *[t.data_ptr() if t is not None else None for t in out], stream)

  for kw in (dict(P=0), dict(P=9), dict(A=0), dict(ptrs=[maps[0].data_ptr()] + [None] * 7), dict(out=(amax, partial, None)),
             dict(out=(None, partial, record))):
    assert step(**kw) == 1, kw
    text = lib.srl_compare_last_error().decode()
    assert text.startswith('srl_compare_step: bad arguments') and '1 <= P <= 8' in text and 'non-null' in text
  torch.cuda.synchronize()
  assert bool((amax == 7).all()) and bool((partial == 7).all()) and bool((record == 7).all())
  with pytest.raises(RuntimeError, match='bad arguments'):
    compare.call('srl_compare_step', amax, 9, *([maps[0]] * 8), 0, B, 1, A, None, amax, partial, record)
  record.zero_()
  assert step() == 0
  torch.cuda.synchronize()
  assert record[0] == B and bool((amax == 1).all())


def test_run_end_to_end_on_the_env(ref_pool):
  from stackrl_amd import compare, env as envs, nets, qops
  from stackrl_amd.baselines import Baseline
  from stackrl_amd.dqn import DQN
  B, L, N, seed = 4, 3, 8, 11
  env = envs.VecStackEnv(n_parallel=B, seed=1, pool=ref_pool, episode_length=L, block=True)
  net = nets.DeepQSiamFCN(env.observation_spec, seed=2).cuda()
  agent = DQN(net, collect_batch_size=B, replay_memory_size=2 * B, seed=9, policy_op=qops.FusedPolicy(chunk=32, fast=True), xcorr='bf16x3')
  policies = {'height': Baseline('height', value=True), 'random': Baseline('random', value=True, seed=3),
              'dqn': lambda obs: agent.greedy(obs, values=True)}
  data = compare.run(env, policies, num_steps=N, seed=seed, keep_values=True)
  P, A = 3, net.n_actions
  T = P * N
  assert data['actions'].shape == (P, T, B, 2) and data['values'].shape == (P, T, B, A) and data['values'].dtype == np.float32
  assert data['rewards'].shape == data['dones'].shape == (P, N, B)
  assert np.array_equal(data['dones'], np.broadcast_to((np.arange(N) % L == L - 1)[None, :, None], (P, N, B)))
  assert np.array_equal(data['action_values'], data['values'].max(-1))
  # the record against the restatement of the kept maps: sums within the reordering bound, counts within the number of values
  # the restatement finds so near a threshold (1e-12 relative) that the order of the threshold's own sums decides their flag
  x = data['values'].reshape(P, T * B, A).astype(np.float64)
  want, _ = compare.compare_reference(x)
  got = data['record']
  n_sums = P + P * (P + 1) // 2
  terms = [np.abs(x[j]).sum() for j in range(P)] + [np.abs(x[i] * x[j]).sum() for i, j in compare.pair_index(P)]
  bound = 2 * (x.shape[1] * A - 1) * U53 * np.array(terms)
  err = np.abs(got[1:1 + n_sums] - want[1:1 + n_sums])
  mu = x.mean(-1, keepdims=True)
  thr2 = mu + x.std(-1, keepdims=True)
  near = sum(int((np.abs(x - t) <= 1e-12 * np.maximum(1.0, np.abs(t))).sum()) for t in (mu, thr2))
  print('sums: largest error / bound', float((err / bound).max()), 'values near a threshold', near,
        'largest count difference', float(np.abs(got[1 + n_sums:] - want[1 + n_sums:]).max()))
  assert got[0] == want[0] == T * B and np.all(err <= bound)
  assert np.all(np.abs(got[1 + n_sums:] - want[1 + n_sums:]) <= near)
  res = compare.analyse(data)
  assert res['corrcoef'].shape == (P, P) and np.allclose(np.diag(res['corrcoef']), 1.0) and np.all(np.diag(res['overlap_mean']) == 1.0)
  assert len(compare.episode_returns(data)[0]) == B * 3              # episodes of 3, 3 and 2 steps in every env
  # each policy's own actions, replayed on a fresh env with the same seed: the recorded rewards and dones, bit for bit
  vw = data['actions'].astype(np.int64)
  fresh = envs.VecStackEnv(n_parallel=B, seed=5, pool=ref_pool, episode_length=L, block=True)
  for p in range(P):
    fresh.seed(seed)
    fresh.reset()
    for t in range(N):
      a = vw[p, p * N + t, :, 0] * int(round(A ** 0.5)) + vw[p, p * N + t, :, 1]
      _, r, d = fresh.step(torch.from_numpy(a).cuda())
      assert np.array_equal(r.cpu().numpy(), data['rewards'][p, t]) and np.array_equal(d.cpu().numpy(), data['dones'][p, t]), (p, t)
      if bool(d.any()):
        fresh.step(torch.zeros(B, dtype=torch.int64, device='cuda'))
  env.close()
  fresh.close()
