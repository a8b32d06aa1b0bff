"""GPU tests of the observation dtypes (env.py:24, :168-180): every dtype's observation equals the reference's `_return`
applied by numpy to the CPU oracle's float maps, bit for bit, the uint32 / uint64 wrap quirk included, while rewards, done
flags, poses and maps are those of the uint8 env.

Expected values: `StackEnv.observation` (env.py:225-231) stacks the height map H and the goal map G (rewarder.py:255-256:
max_z - object_max_dimension inside the goal rectangle, 0 outside) and applies `_return`; the object maps go through the same
`_return`.  H, the object maps and the goal rectangle are the oracle's (`OracleEnv.maps()`).  Every check first asserts that
the uint8 form of that construction is the oracle's own uint8 observation, so the expected values are built from the right
source."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

DTYPES = ('uint8', 'uint16', 'uint32', 'uint64', 'float16', 'float32', 'float64')
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
CENTRE = 48 * 97 + 48          # the centre pixel of the 97 x 97 action map (128 - 32 + 1)


def _return(x, dtype, den):
  """`StackEnv._return` (env.py:171-180) as numpy evaluates it: x * (2^k - 1) / den in float32, then the cast."""
  k = {'uint8': 8, 'uint16': 16, 'uint32': 32, 'uint64': 64}.get(dtype)
  with np.errstate(invalid='ignore', over='ignore'):
    if k:
      return np.array(x * (2 ** k - 1) / den, dtype=dtype)
    return np.array(x, dtype=dtype)


def _expected(cfg, o, dtype):
  H, O, g = o.maps()
  den = max(cfg.max_z, cfg.object_max_dimension)
  G = np.zeros_like(H)
  for i in range(len(g)):
    u, v, h, w = g[i]
    G[i, u:u + h, v:v + w] = np.float32(cfg.max_z - cfg.object_max_dimension)
  return _return(np.stack([H, G], -1), dtype, den), _return(O[..., None], dtype, den), H


def _bits(a):
  return a.view(BITS[a.dtype.itemsize])


def _check_obs(gobs, o, oobs, cfg, dtype, tag):
  """gobs: the dtype env's observation (tensors); oobs: the oracle's own uint8 observation."""
  from stackrl_amd.env import TORCH_DTYPES
  um, uo, H = _expected(cfg, o, 'uint8')
  assert np.array_equal(um, oobs[0]) and np.array_equal(uo, oobs[1]), tag + ': the expected values are not built right'
  em, eo, _ = _expected(cfg, o, dtype)
  for name, t, e in (('obs_map', gobs[0], em), ('obs_obj', gobs[1], eo)):
    assert t.dtype == TORCH_DTYPES[dtype], '{}: {} has dtype {}'.format(tag, name, t.dtype)
    got = t.cpu().numpy()
    assert got.dtype == e.dtype and got.shape == e.shape, '{}: {} {} {}'.format(tag, name, got.dtype, got.shape)
    bad = _bits(got) != _bits(e)
    assert not bad.any(), '{}: {} differs at {} elements, first {}: {} vs {}'.format(
      tag, name, int(bad.sum()), np.argwhere(bad)[0].tolist(), got[bad][0], e[bad][0])
  return H


def _same_step(a, b, tag):
  """rewards, done flags and the telemetry of two handles, bit for bit"""
  assert np.array_equal(a[1].cpu().numpy().view(np.uint32), b[1].cpu().numpy().view(np.uint32)), tag + ': reward'
  assert torch.equal(a[2], b[2]), tag + ': done'


def _same_state(g, u, tag):
  for k, (x, y) in enumerate(zip(g.state(), u.state())):
    assert np.array_equal(_bits(x), _bits(y)), '{}: state {}'.format(tag, k)
  for k, (x, y) in enumerate(zip(g.maps(), u.maps())):
    assert np.array_equal(_bits(x), _bits(y)), '{}: maps {}'.format(tag, k)


def _script(rng, n, L, pool):
  ids = np.stack([rng.choice(len(pool), size=L, replace=False) for _ in range(n)]).astype(np.int32)
  rect = np.stack([[rng.randint(8, 40), rng.randint(8, 40), 64, 64] for _ in range(n)]).astype(np.int32)
  return ids, rect


@pytest.mark.parametrize('dtype', DTYPES)
def test_scripted_episodes_in_every_dtype(ref_pool, oracle_mod, dtype):
  """The script of test_parity_gpu.py::test_scripted_episodes (32 envs x 8 rocks) through done and the auto-reset step: the
  dtype handle's observations are `_return` of the oracle's maps; a uint8 handle on the same script has the same rewards,
  done flags, state and maps."""
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  n, L = 32, 8
  g = envs.VecStackEnv(n_parallel=n, seed=11, pool=ref_pool, block=True, episode_length=L, dtype=dtype)
  u = envs.VecStackEnv(n_parallel=n, seed=11, pool=ref_pool, block=True, episode_length=L)
  cfg = StackConfig(n_envs=n, episode_length=L, dtype=dtype)
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=11)
  assert g.observation_spec[0].dtype == getattr(torch, dtype) and g.observation_spec[1].dtype == getattr(torch, dtype)
  rng = np.random.RandomState(5)
  ids, rect = _script(rng, n, L, ref_pool)
  for e in (g, u, o):
    e.set_script(ids, rect)
  gout, uout, oout = g.reset(), u.reset(), o.reset()
  _check_obs(gout[0], o, oout[0], cfg, dtype, 'reset')
  _same_state(g, u, 'reset')
  for k in range(L + 2):
    a = rng.randint(0, g.n_actions, size=n).astype(np.int64)
    gout = g.step(torch.from_numpy(a).cuda())
    uout = u.step(torch.from_numpy(a).cuda())
    oout = o.step(a)
    tag = '{} step {}'.format(dtype, k)
    _check_obs(gout[0], o, oout[0], cfg, dtype, tag)
    assert torch.equal(uout[0][0].cpu(), torch.from_numpy(oout[0][0])), tag + ': uint8 handle'
    _same_step(gout, uout, tag)
    _same_state(g, u, tag)
    if k == L - 1:
      assert oout[2].all() and gout[2].all()
    if k == L:
      assert not oout[2].any() and not gout[2].any()
  for e in (g, u):
    e.close()


@pytest.mark.parametrize('dtype', ['uint32', 'uint64'])
def test_wrap_quirk_at_the_top_of_the_window(ref_pool, oracle_mod, dtype):
  """float32(2^k - 1) = 2^k for k = 32, 64: a height of exactly den gives y = 2^k, which numpy (x86-64) turns into 0.  With
  max_z = 0.125 (den = max_z) and every rock dropped on the centre pixel the pile reaches the top of the window, where the
  height map saturates at max_z: those pixels must exist, hold 0, and everything else must equal numpy."""
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  n, L, max_z = 8, 8, 0.125
  g = envs.VecStackEnv(n_parallel=n, seed=11, pool=ref_pool, block=True, episode_length=L, max_z=max_z, dtype=dtype)
  cfg = StackConfig(n_envs=n, episode_length=L, max_z=max_z, dtype=dtype)
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=11)
  rng = np.random.RandomState(5)
  ids, rect = _script(rng, n, L, ref_pool)
  g.set_script(ids, rect); o.set_script(ids, rect)
  gout, oout = g.reset(), o.reset()
  _check_obs(gout[0], o, oout[0], cfg, dtype, 'reset')
  a = np.full(n, CENTRE, np.int64)
  top_total = 0
  for k in range(L):
    gout = g.step(torch.from_numpy(a).cuda())
    oout = o.step(a)
    tag = '{} step {}'.format(dtype, k)
    H = _check_obs(gout[0], o, oout[0], cfg, dtype, tag)
    top = H == np.float32(max_z)
    got = gout[0][0].cpu().numpy()[..., 0]
    print(tag, 'pixels at max_z', int(top.sum()))
    assert (got[top] == 0).all(), tag
    top_total += int(top.sum())
  assert top_total > 0, 'the pile never reached max_z: the case is vacuous'
  g.close()


PLANE_CAP = 640                # SRL_PLANE_CAP (csrc/render.hip): plane / side slots of one rock group


@pytest.mark.parametrize('dtype,kw,n,L', [
  ('uint16', dict(resolution_factor=3), 6, 5),        # 32 x 32 map (1,024 pixels < 4 x 512 threads): the general walk with its
  ('float64', dict(resolution_factor=3), 6, 5),       #   bound on the group index
  ('uint16', dict(observable_size_ratio=3), 6, 5),    # 96 x 96 map: the general walk, whose groups change columns
  ('float64', dict(observable_size_ratio=3), 6, 5),
  ('float64', {}, 4, 14),                             # 14 rocks hold more slots than PLANE_CAP: a second rock group
])
def test_general_walk_and_later_groups_in_other_dtypes(ref_pool, oracle_mod, dtype, kw, n, L):
  """The render kernel's stores of a type other than uint8 (element sizes 2 and 8) where the default 128 x 128 map with one
  rock group does not take them: the early stores and the epilogue on the general pixel-group walk (maps whose width does not
  divide 4 x 512, and maps smaller than one round of the workgroup), and the epilogue after a later rock group.  Every
  observation through done and the auto-reset step is `_return` of the oracle's maps, bit for bit; rewards and done flags
  are the oracle's."""
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  seed = 31
  g = envs.VecStackEnv(n_parallel=n, seed=seed, pool=ref_pool, block=True, episode_length=L, dtype=dtype, **kw)
  cfg = StackConfig(n_envs=n, episode_length=L, dtype=dtype, **kw)
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=seed)
  res = 2 ** kw.get('resolution_factor', 5) * kw.get('observable_size_ratio', 4)
  assert g.observation_spec[0].shape == (res, res, 2) and g.observation_spec[0].dtype == getattr(torch, dtype)
  gout, oout = g.reset(), o.reset()
  _check_obs(gout[0], o, oout[0], cfg, dtype, 'reset')
  most_slots = 0
  for k in range(L + 1):
    a = g.sample()
    assert np.array_equal(a.cpu().numpy(), o.sample())
    gout = g.step(a)
    oout = o.step(a.cpu().numpy())
    tag = '{} {} step {}'.format(dtype, kw, k)
    _check_obs(gout[0], o, oout[0], cfg, dtype, tag)
    np.testing.assert_allclose(gout[1].cpu().numpy(), oout[1], rtol=0, atol=1e-7, err_msg=tag + ': reward')   # (test_parity_gpu's bound)
    assert np.array_equal(gout[2].cpu().numpy(), oout[2]), tag + ': done'
    hdr, nb = g.stage_records().view(np.int32)[:, :, 0], g.state()[1]    # per rock: ..., up-facing planes, outline sides
    most_slots = max([most_slots] + [int(hdr[e, :int(nb[e]), 2:4].sum()) for e in range(n)])
  if L == 14:
    assert most_slots > PLANE_CAP, 'no env held more than one rock group ({} slots): the case is vacuous'.format(most_slots)
  g.close()


@pytest.mark.parametrize('dtype', ['float32', 'uint16'])
@pytest.mark.parametrize('ordering', [False, True])
def test_stack_v2_object_maps_in_other_dtypes(ref_pool, oracle_mod, dtype, ordering):
  """Stack-v2 (orientation_freedom = 3: eight maps per rock), with and without ordering freedom (the maps of every unplaced
  rock, then empty maps): obs_obj converted from the float cache, the empty maps included."""
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  n, L, seed = 6, 6, 21
  kw = dict(orientation_freedom=3, ordering_freedom=ordering)
  g = envs.make('Stack-v2', n_parallel=n, seed=seed, pool=ref_pool, block=True, episode_length=L, dtype=dtype, **kw)
  cfg = StackConfig(n_envs=n, episode_length=L, dtype=dtype, **kw)
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=seed)
  assert g.observation_spec[1].shape == ((L if ordering else 1) * 8, 32, 32, 1)
  gout, oout = g.reset(), o.reset()
  _check_obs(gout[0], o, oout[0], cfg, dtype, 'reset')
  empty_seen = 0
  for t in range(L + 2):
    a = g.sample()
    assert np.array_equal(a.cpu().numpy(), o.sample())
    gout = g.step(a)
    oout = o.step(a.cpu().numpy())
    _check_obs(gout[0], o, oout[0], cfg, dtype, '{} step {}'.format(dtype, t))
    assert np.array_equal(gout[1].cpu().numpy(), oout[1]) and np.array_equal(gout[2].cpu().numpy(), oout[2])
    empty_seen += int((o.maps()[1].reshape(n, -1, 32 * 32) == o.maps()[1].min()).all(-1).sum())
  if ordering:
    assert empty_seen > 0
  g.close()


def test_pipelined_float32_equals_one_handle_and_stack_v1_carries_the_dtype(ref_pool, oracle_mod):
  """make('Stack-v0', groups=2, dtype='float32') (PipelinedVecStackEnv) equals the one-handle float32 env bit for bit;
  make('Stack-v1', dtype='uint16') steps with uint16 observations (its start placements by a given policy: the default one
  runs the uint8 heuristic kernels) and otherwise follows its uint8 twin."""
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  B, L, seed = 12, 8, 31
  a = envs.make('Stack-v0', n_parallel=B, seed=seed, pool=ref_pool, episode_length=L, dtype='float32')
  p = envs.make('Stack-v0', n_parallel=B, seed=seed, pool=ref_pool, episode_length=L, groups=2, dtype='float32')
  cfg = StackConfig(n_envs=B, episode_length=L, dtype='float32')
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=seed)
  assert p.groups == 2 and p.observation_spec[0].dtype == torch.float32
  sa, sp, so = a.reset()(), p.reset()(), o.reset()
  for t in range(L + 2):
    tag = 'call {}'.format(t)
    for x, y in zip(sa[0], sp[0]):
      assert x.dtype == y.dtype == torch.float32 and torch.equal(x.view(torch.int32), y.view(torch.int32)), tag
    _check_obs(sp[0], o, so[0], cfg, 'float32', tag)
    _same_step(sa, sp, tag)
    act = a.sample()
    assert torch.equal(act, p.sample()) and np.array_equal(act.cpu().numpy(), o.sample())
    sa, sp, so = a.step(act)(), p.step(act)(), o.step(act.cpu().numpy())
  for e in (a, p):
    e.close()

  def centre(obs):
    return torch.full((obs[0].shape[0],), CENTRE, dtype=torch.int64, device=obs[0].device)

  n, L, N = 4, 3, 5
  v = envs.make('Stack-v1', n_parallel=n, seed=7, pool=ref_pool, block=True, episode_length=L, n_objects=N, dtype='uint16',
                start_policy=centre)
  w = envs.make('Stack-v1', n_parallel=n, seed=7, pool=ref_pool, block=True, episode_length=L, n_objects=N, start_policy=centre)
  assert v.observation_spec[0].dtype == v.observation_spec[1].dtype == torch.uint16
  sv, sw = v.reset(), w.reset()
  den = max(v.config.max_z, v.config.object_max_dimension)
  for t in range(L + 2):
    for x in sv[0]:
      assert x.dtype == torch.uint16 and x.shape[0] == n
    H = v.maps()[0]
    assert np.array_equal(sv[0][0].cpu().numpy()[..., 0], _return(H, 'uint16', den)), 'call {}'.format(t)
    _same_step(sv, sw, 'Stack-v1 call {}'.format(t))
    _same_state(v, w, 'Stack-v1 call {}'.format(t))
    act = w.sample()
    sv, sw = v.step(act), w.step(act)
  for e in (v, w):
    e.close()


def test_float32_under_the_concurrent_rollout_forward_equals_the_oracle(oracle_mod):
  """The pattern of test_parity_gpu.py::test_env_step_under_the_concurrent_rollout_forward_equals_the_oracle, one small
  shape: the float32 env steps on a side stream while the Q-net's kernels run on the current one (DESIGN.md section 6a:
  the render kernel's new code paths face the same check as the old ones); every observation is the oracle's float32 cast
  and rewards, done flags, state and height maps are the oracle's, bit for bit."""
  from stackrl_amd import assets, env as envs, nets, qops
  from stackrl_amd.config import StackConfig
  B, L, seed = 256, 8, 5
  pool = assets.default_pool()
  e = envs.make('Stack-v0', n_parallel=B, seed=seed, pool=pool, episode_length=L, side_stream=True, dtype='float32')
  cfg = StackConfig(n_envs=B, episode_length=L, dtype='float32')
  o = oracle_mod.OracleEnv(cfg, pool, seed=seed)
  u8 = (envs.TensorSpec((128, 128, 2), torch.uint8), envs.TensorSpec((32, 32, 1), torch.uint8))
  net = nets.DeepQSiamFCN(u8, seed=2).cuda()
  pol = qops.FusedPolicy(chunk=256, fast=True)
  gen = torch.Generator(device='cuda').manual_seed(1)
  x = (torch.randint(0, 256, (B, 128, 128, 2), generator=gen, device='cuda', dtype=torch.uint8),
       torch.randint(0, 256, (B, 32, 32, 1), generator=gen, device='cuda', dtype=torch.uint8))
  e.reset()()
  o.reset()
  bad = []
  for t in range(L + 1):
    a = e.sample()
    ao = o.sample()
    assert np.array_equal(a.cpu().numpy(), ao)
    w = e.step(a, block=False)
    for _ in range(2):
      pol(net, x, 1.0, gen)                   # the forward while the step is in flight
    (om, oo), r, d = w()
    (omo, ooo), ro, do = o.step(ao)
    try:
      _check_obs((om, oo), o, (omo, ooo), cfg, 'float32', 'call {}'.format(t))
      ok = True
    except AssertionError as ex:
      ok = False
      print(ex)
    gs, os_ = e.state(), o.state()
    same = (ok and np.array_equal(r.cpu().numpy().view(np.uint32), ro.view(np.uint32)) and np.array_equal(d.cpu().numpy(), do)
            and all(np.array_equal(_bits(x_), _bits(y_)) for x_, y_ in zip(gs, os_))
            and np.array_equal(_bits(e.maps()[0]), _bits(o.maps()[0])))
    if not same:
      bad.append(t)
  e.close()
  assert not bad, 'float32 env results under the concurrent forward differ from the oracle at calls {}'.format(bad)


def test_training_setup_refuses_a_float32_env(ref_pool):
  from stackrl_amd import baselines, env as envs, nets
  from stackrl_amd.dqn import DQN
  from stackrl_amd.training import Trainer
  env = envs.make('Stack-v0', n_parallel=4, seed=3, pool=ref_pool, episode_length=4, dtype='float32')
  (om, oo), _, _ = env.reset(block=True)
  with pytest.raises(ValueError, match='float32'):
    baselines.heuristic_values('height', (om, oo))
  u8 = (envs.TensorSpec((128, 128, 2), torch.uint8), envs.TensorSpec((32, 32, 1), torch.uint8))
  agent = DQN(nets.DeepQSiamFCN(u8, seed=1).cuda(), collect_batch_size=4, replay_memory_size=16, seed=7)
  with pytest.raises(ValueError, match='float32'):
    Trainer(env, agent)
  env.close()
