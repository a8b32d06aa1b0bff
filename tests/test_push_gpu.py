"""GPU tests of the push test (csrc/push.hip; include/stackrl_hip.h "Push test"; stackrl_amd/push.py): `srl_poses` against
`srl_get_state`, `srl_kick` and `srl_pose_distances` against the numpy restatement of tests/push_cases.py, an in-place push
against the CPU oracle, `PushTest`, the lookahead with a push, the other env classes and the refusals.  Every comparison is
bit for bit (a NaN on both sides counts as equal: push_cases.same_bits)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import push_cases as pc
import settle_scenarios as S
from contact_cases import HDR_PAD, offsets
from state_cases import blob_words

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 5
KW = dict(resolution_factor=4)
TOL = (1e-4, 1e-3)
SUBSTEPS = 20


def _mk(ref_pool, L, n=N, seed=5, cls=None, **kw):
  from stackrl_amd import env as envs
  args = dict(KW, **kw)
  return (cls or envs.VecStackEnv)(n_parallel=n, seed=seed, pool=ref_pool, block=True, episode_length=L, **args)


def _cuda(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _centre(g, n=N):
  aw = g.config.overhead_res - g.config.object_res + 1
  return torch.full((n,), (aw // 2) * aw + aw // 2, dtype=torch.int64, device='cuda')


def _staggered(g, steps, n=N):
  """`steps` calls in which env e places a rock only while e > call index: env e ends with min(e, steps) rocks."""
  from stackrl_amd.config import ACTION_HOLD
  for t in range(steps):
    a = _centre(g, n)
    a[:t + 1] = ACTION_HOLD
    g.step(a)


def _host(g):
  """(poses [B, L, 8], body counts, velocities [B, L, 8]) through the blocking host copies."""
  L = g.config.episode_length
  p, nb, _, _ = g.state()
  return p[:, :L].copy(), nb.copy(), g.velocities()[:, :L].copy()


def _places(g):
  L = g.config.episode_length
  return [pc.place_poses(r, L) for r in g.get_state().records.cpu().numpy()]


def _assert_restated(d, poses, vel, nb, places, ref=None, ref_nb=None, tol=TOL, tag=''):
  d = d.cpu()
  for e in range(len(nb)):
    rows, summary = pc.rows_summary(poses[e], vel[e], nb[e], places[e], None if ref is None else ref[e],
                                    None if ref_nb is None else ref_nb[e], tol)
    assert pc.same_bits(d.rows[e].numpy(), rows), (tag, e, d.rows[e].numpy(), rows)
    assert pc.same_bits(d.summary[e].numpy(), summary), (tag, e, d.summary[e].numpy(), summary)


def _same_distances(x, y):
  x, y = x.cpu(), y.cpu()
  return pc.same_bits(x.rows.numpy(), y.rows.numpy()) and pc.same_bits(x.summary.numpy(), y.summary.numpy())


# ------------------------------------------------------------------------------------------------ 1. srl_poses
@pytest.mark.parametrize('n,L', [(1, 8), (5, 8), (5, 9), (5, 32)])
def test_poses_equal_get_state(ref_pool, n, L):
  g = _mk(ref_pool, L, n=n)

  def check(tag, want_nb):
    out = (torch.full((n, L, 8), 7.5, dtype=torch.float32, device='cuda'), torch.full((n,), -5, dtype=torch.int32, device='cuda'))
    poses, nb = g.poses(out=out)
    assert poses.data_ptr() == out[0].data_ptr()
    hp, hnb, _, _ = g.state()
    assert np.array_equal(nb.cpu().numpy(), hnb) and list(hnb) == [want_nb] * n, tag
    got = poses.cpu().numpy()
    assert np.array_equal(got[:, :, :7].view(np.int32), hp[:, :L, :7].view(np.int32)), tag
    assert np.array_equal(got[:, :, 7].view(np.int32), hp[:, :L, 7].astype(np.int32)), tag     # the id: int32 bits here, a float there
    assert not got[:, want_nb:].view(np.int32).any(), tag                                       # zero rows at or above nb
    fresh, fresh_nb = g.poses()
    assert torch.equal(fresh.view(torch.int32), poses.view(torch.int32)) and torch.equal(fresh_nb, nb)
  g.reset()
  check('after reset', 0)
  a = _centre(g, n)
  g.step(a)
  check('after one step', 1)
  if L == 8:
    for _ in range(L - 1):
      g.step(a)
    check('pile full', L)
  g.close()


# ------------------------------------------------------------------------------------------------ 2. srl_kick
def test_kick_equals_the_restatement_and_changes_nothing_else(ref_pool):
  from stackrl_amd.config import ACTION_HOLD
  L = 8
  g = _mk(ref_pool, L)
  g.reset()
  _staggered(g, 3)
  rec0 = g.get_state().records.cpu().numpy()
  _, nb, v = _host(g)
  assert list(nb) == [0, 1, 2, 3, 3]
  rng = np.random.RandomState(1)
  codes = {'all': pc.KICK_ALL, 'last': pc.KICK_LAST}
  # both layouts x the three selections; slot 1 is below nb in three envs, slot 2 in two, slots 3 and L - 1 in none
  for per_body, select in [(1, 'all'), (0, 'all'), (1, 'last'), (0, 'last'), (1, 1), (0, 2), (1, 3), (0, L - 1), (1, 0)]:
    dv = rng.normal(size=(N, L, 8) if per_body else (N, 8)).astype(F32)
    g.kick(_cuda(dv), select)
    want = np.stack([pc.kick(v[e], nb[e], dv[e], per_body, codes.get(select, select)) for e in range(N)])
    got = g.velocities()[:, :L]
    assert pc.same_bits(got, want), (per_body, select)
    assert (select in (3, L - 1)) == pc.same_bits(want, v), (per_body, select)
    v = want
  # the 3-column forms: linear increments only
  for shape in [(N, 3), (N, L, 3)]:
    dv3 = rng.normal(size=shape).astype(F32)
    wide = np.zeros(shape[:-1] + (8,), F32)
    wide[..., :3] = dv3
    g.kick(_cuda(dv3))
    want = np.stack([pc.kick(v[e], nb[e], wide[e], int(len(shape) == 3), pc.KICK_ALL) for e in range(N)])
    assert pc.same_bits(g.velocities()[:, :L], want), shape
    v = want
  # every other word of the blob: a call in which every env holds leaves the blobs alone and makes the records readable again
  g.step(torch.full((N,), ACTION_HOLD, dtype=torch.int64, device='cuda'))
  rec1 = g.get_state().records.cpu().numpy()
  o = offsets(L)[0]
  words = slice(HDR_PAD, HDR_PAD + blob_words(L))
  want = rec0[:, words].copy()
  for e in range(N):
    vw = want[e].view(F32)[o['V']:o['V'] + 8 * L].reshape(L, 8)
    for b in range(nb[e]):
      vw[b, 0:6:2], vw[b, 1:6:2] = v[e, b, 0:3], v[e, b, 4:7]
  assert np.array_equal(rec1[:, words], want) and np.array_equal(rec1[:, 0], nb)
  assert not np.array_equal(rec1[1:, words], rec0[1:, words])
  g.close()


# ------------------------------------------------------------------------------------------------ 3. srl_pose_distances
def test_distances_equal_the_restatement(ref_pool):
  L = 8
  g = _mk(ref_pool, L)
  g.reset()
  _staggered(g, 3)
  poses, nb, vel = _host(g)
  _assert_restated(g.distances(tol=TOL), poses, vel, nb, _places(g), tag='from place')
  # a reference taken before a step: `Simulator.distances` of that step; every env's new rock is measured from its place pose
  before = g.poses()
  g.step(_centre(g))
  poses1, nb1, vel1 = _host(g)
  assert list(nb1) == [1, 2, 3, 4, 4]
  d = g.distances(since=before, tol=TOL)
  _assert_restated(d, poses1, vel1, nb1, _places(g), ref=poses, ref_nb=nb, tag='since')
  d = d.cpu()
  assert any(float(d.perr[e, nb[e]]) > 0 for e in range(N)) and not bool(d.rows[0, 1:].any())
  assert torch.equal(d.nb, torch.from_numpy(nb1.astype(F32))) and bool((d.moved <= d.nb).all())
  assert torch.equal(d.at_rest, d.max_speed <= g.config.velocity_threshold) and torch.equal(d.max_perr, d.perr.max(1).values)
  assert torch.equal(d.sum_perr, d.summary[:, 4]) and torch.equal(d.min_dz, d.dz.min(1).values.clamp(max=0))
  # without the counts every row of the reference counts (the new rock's is a zero row: it is that far from the origin)
  _assert_restated(g.distances(since=(before[0], None), tol=TOL), poses1, vel1, nb1, _places(g), ref=poses, ref_nb=None, tag='no counts')
  # `out`: filled in place, rows of the slots at or above nb zeroed
  from stackrl_amd.push import PoseDistances
  out = PoseDistances(torch.full((N, L, 4), 7.5, device='cuda'), torch.full((N, 8), 7.5, device='cuda'), 0.01)
  assert _same_distances(g.distances(since=before, tol=TOL, out=out), d) and out.rows.data_ptr() == g.distances(out=out).rows.data_ptr()
  g.close()


def test_distances_of_a_step_equal_the_oracle(ref_pool, oracle_mod):
  """The oracle's poses before and after the same scripted step through `srlo_distance_from_place`."""
  from stackrl_amd.config import StackConfig
  L, n = 8, 4
  g = _mk(ref_pool, L, n=n, seed=S.ENV_SEED)
  o = oracle_mod.OracleEnv(StackConfig(n_envs=n, episode_length=L, **KW), ref_pool, seed=S.ENV_SEED)
  ids, rect, rng = S.pile_script(len(ref_pool), n, L)
  g.set_script(ids, rect); o.set_script(ids, rect)
  g.reset(); o.reset()
  aw = g.config.overhead_res - g.config.object_res + 1
  lib = oracle_mod.lib()
  compared = 0
  for t in range(4):
    a = S.pile_actions(rng, n, aw)
    before, (ob, onb, _, _) = g.poses(), o.state()
    o.step(a); g.step(_cuda(a))
    d = g.distances(since=before, tol=TOL).cpu()
    oa = o.state()[0]
    for e in range(n):
      for b in range(onb[e]):
        want = np.zeros(2, F32)
        lib.srlo_distance_from_place(np.ascontiguousarray(ob[e, b, :7]).ctypes.data_as(ctypes.c_void_p),
                                     np.ascontiguousarray(oa[e, b, :7]).ctypes.data_as(ctypes.c_void_p), want.ctypes.data_as(ctypes.c_void_p))
        assert pc.same_bits(d.rows[e, b, :2].numpy(), want), (t, e, b)
        assert d.rows[e, b, 2] == F32(oa[e, b, 2] - ob[e, b, 2])
        compared += 1
  assert compared == n * 6
  g.close(); o.close()


def test_a_nan_pose_counts_as_moved(ref_pool):
  L = 8
  g = _mk(ref_pool, L)
  g.reset()
  _staggered(g, 3)
  places = _places(g)
  p = g.state()[0].copy()
  p[3, 1, 0] = np.nan
  g.set_body_state(p, None)
  poses, nb, vel = _host(g)
  assert np.isnan(poses[3, 1, 0])
  d = g.distances(tol=(10.0, 10.0))
  _assert_restated(d, poses, vel, nb, places, tol=(10.0, 10.0), tag='nan')
  d = d.cpu()
  assert d.moved.tolist() == [0, 0, 0, 1, 0] and bool(torch.isnan(d.perr[3, 1])) and bool(torch.isnan(d.sum_perr[3]))
  assert not bool(torch.isnan(d.max_perr).any())
  g.close()


# ------------------------------------------------------------------------------------------------ 4. a push against the oracle
@pytest.mark.parametrize('L,kernel', [(8, 0), (9, 1), (32, 2)])
def test_in_place_push_equals_the_oracle(ref_pool, oracle_mod, L, kernel):
  from stackrl_amd.config import StackConfig
  n = 4
  g = _mk(ref_pool, L, n=n, seed=S.ENV_SEED)
  o = oracle_mod.OracleEnv(StackConfig(n_envs=n, episode_length=L, **KW), ref_pool, seed=S.ENV_SEED)
  assert g.step_variant()[2] == kernel
  ids, rect, rng = S.pile_script(len(ref_pool), n, L)
  g.set_script(ids, rect); o.set_script(ids, rect)
  g.reset(); o.reset()
  aw = g.config.overhead_res - g.config.object_res + 1
  for _ in range(3):
    a = S.pile_actions(rng, n, aw)
    o.step(a); g.step(_cuda(a))
  places = _places(g)
  poses0, nb, _ = _host(g)
  dv = np.zeros((n, L, 8), F32)
  dv[..., 0:3] = rng.normal(scale=0.15, size=(n, L, 3))
  dv[..., 4:7] = rng.normal(scale=1.0, size=(n, L, 3))
  d = g.push(_cuda(dv), SUBSTEPS, tol=TOL)
  ov = o.velocities()
  for e in range(n):
    ov[e, :L] = pc.kick(ov[e, :L], nb[e], dv[e], 1, pc.KICK_ALL)        # one float32 addition per component
  o.set_body_state(None, ov)
  o.step_simulation(SUBSTEPS)
  poses1, nb1, vel1 = _host(g)
  assert list(nb) == [3] * n and np.array_equal(nb1, nb)
  assert pc.same_bits(poses1[..., :7], o.state()[0][:, :L, :7]), np.abs(poses1[..., :7] - o.state()[0][:, :L, :7]).max()
  assert pc.same_bits(vel1, o.velocities()[:, :L]), np.abs(vel1 - o.velocities()[:, :L]).max()
  _assert_restated(d, poses1, vel1, nb1, places, ref=poses0, ref_nb=nb, tag='push')
  assert float(d.max_perr.min()) > 0
  g.close(); o.close()


# ------------------------------------------------------------------------------------------------ 5. PushTest
def test_push_test_forks_and_leaves_the_env_alone(ref_pool):
  from stackrl_amd.push import PushSpec, PushTest
  L, B, k = 8, 4, 3
  g = _mk(ref_pool, L, n=B)
  h = _mk(ref_pool, L, n=B, seed=77)
  pt = PushTest(g, trials=k)
  g.reset()
  a = _centre(g, B)
  for _ in range(3):
    g.step(a)
  state = g.get_state()
  rng = np.random.RandomState(2)
  one = np.zeros((B, 1, 8), F32)
  one[..., 0:2] = rng.normal(scale=0.3, size=(B, 1, 2))
  d = pt.evaluate(_cuda(np.repeat(one, k, axis=1)), substeps=SUBSTEPS, tol=TOL)
  assert tuple(d.rows.shape) == (B, k, L, 4) and tuple(d.summary.shape) == (B, k, 8) and tuple(d.moved.shape) == (B, k)
  assert torch.equal(g.get_state().records, state.records)                 # `env` is not touched
  for j in range(1, k):                                                    # the same push in another slot: the same result
    assert pc.same_bits(d.rows[:, j].cpu().numpy(), d.rows[:, 0].cpu().numpy()) and pc.same_bits(d.summary[:, j].cpu().numpy(), d.summary[:, 0].cpu().numpy())
  assert float(d.max_perr.min()) > 0
  # a trial = an in-place push of a forked copy
  h.set_state(state)
  dh = h.push(_cuda(one[:, 0]), SUBSTEPS, tol=TOL)
  assert pc.same_bits(dh.rows.cpu().numpy(), d.rows[:, 0].cpu().numpy()) and pc.same_bits(dh.summary.cpu().numpy(), d.summary[:, 0].cpu().numpy())
  # a PushSpec: its draw, its selection and its tolerances
  for mode in ('bump', 'shake', 'last'):
    spec = PushSpec(speed=0.3, substeps=10, mode=mode, tol=TOL, seed=4)
    dv = spec.draw(B, k, L, 'cuda')
    assert tuple(dv.shape) == ((B, k, L, 8) if mode == 'shake' else (B, k, 8))
    x, y = pt.evaluate(spec), pt.evaluate(dv, substeps=10, select='last' if mode == 'last' else 'all', tol=TOL)
    assert _same_distances(x, y), mode
    assert not _same_distances(x, d)
  assert torch.equal(g.get_state().records, state.records)
  g.step(a)                                                                # and the env goes on
  pt.close(); g.close(); h.close()


def test_push_test_follows_set_pool(ref_pool):
  from stackrl_amd.push import PushSpec, PushTest
  L, B, k = 4, 4, 2
  g = _mk(ref_pool, L, n=B)
  pt = PushTest(g, trials=k)
  spec = PushSpec(speed=0.2, substeps=8, mode='bump', tol=TOL, seed=1)
  g.reset()
  g.step(_centre(g, B))
  pt.evaluate(spec)
  other = ref_pool.subset(list(range(len(ref_pool) - 1, 0, -1)))
  g.set_pool(other)
  with pytest.raises(RuntimeError, match='needs a reset first'):
    pt.evaluate(spec)
  g.seed(5)
  g.reset()
  g.step(_centre(g, B))
  d = pt.evaluate(spec)
  assert pt.scratch.pool is other
  fresh = PushTest(g, trials=k)
  assert _same_distances(fresh.evaluate(spec), d) and float(d.nb.min()) == 1
  fresh.close(); pt.close(); g.close()


# ------------------------------------------------------------------------------------------------ 6. the lookahead with a push
def test_lookahead_with_a_push(ref_pool):
  from stackrl_amd import env as envs
  from stackrl_amd.baselines import Baseline
  from stackrl_amd.lookahead import Lookahead, LookaheadPolicy, score
  from stackrl_amd.push import PushSpec
  n, L, k = 4, 6, 3
  g = envs.VecStackEnv(n_parallel=n, seed=2, pool=ref_pool, block=True, episode_length=L)
  h = envs.VecStackEnv(n_parallel=n, seed=9, pool=ref_pool, block=True, episode_length=L)
  look = Lookahead(g, k)
  base = Baseline('height', value=True)
  spec = PushSpec(speed=0.2, substeps=10, mode='bump', seed=3)
  plain, pushed, strict = LookaheadPolicy(base, look), LookaheadPolicy(base, look, push=spec, penalty=0.0), LookaheadPolicy(base, look, push=spec, penalty=0.5)
  obs = g.reset()[0]
  for t in range(3):
    a0, _ = plain(obs)
    a1, _ = pushed(obs)
    assert torch.equal(a0, a1), t                                          # penalty 0: the choice of the policy without a push
    cand, reward = pushed.last
    assert torch.equal(cand, plain.last[0]) and torch.equal(reward.view(torch.int32), plain.last[1].view(torch.int32))
    dist = pushed.last_push
    assert tuple(dist.moved.shape) == (n, k) and bool((dist.nb == t + 1).all())
    a2, _ = strict(obs)
    assert torch.equal(a2, cand.gather(1, torch.sort(score(strict.last[1], strict.last_push, 0.5), dim=1, descending=True, stable=True).indices[:, :1])[:, 0])
    if t == 1:                                                             # the distances are those of a push after that step
      state = g.get_state()
      dv = spec.draw(n, k, L, 'cuda')
      for j in range(k):
        h.set_state(state)
        h.step(cand[:, j])
        dh = h.push(dv[:, j], spec.substeps, tol=spec.tol)
        assert pc.same_bits(dh.rows.cpu().numpy(), dist.rows[:, j].cpu().numpy()) and pc.same_bits(dh.summary.cpu().numpy(), dist.summary[:, j].cpu().numpy()), j
    obs = g.step(a0)[0]
  look.close(); g.close(); h.close()


# ------------------------------------------------------------------------------------------------ 7. the other env classes
def _push_against_restatement(g, rng, select='all'):
  L, B = g.config.episode_length, g.batch_size
  places = _places(g)
  poses0, nb0, _ = _host(g)
  dp, dnb = g.poses()
  assert np.array_equal(dnb.cpu().numpy(), nb0) and pc.same_bits(dp.cpu().numpy()[..., :7], poses0[..., :7])
  dv = rng.normal(scale=0.2, size=(B, L, 8)).astype(F32)
  d = g.push(_cuda(dv), 10, select=select, tol=TOL)
  poses1, nb1, vel1 = _host(g)
  _assert_restated(d, poses1, vel1, nb1, places, ref=poses0, ref_nb=nb0, tag=type(g).__name__)
  return d


def test_started_env_and_stack_v2(ref_pool):
  from stackrl_amd import env as envs
  rng = np.random.RandomState(6)
  s = envs.StartedVecStackEnv(n_parallel=4, seed=3, pool=ref_pool, block=True, episode_length=2, n_objects=4)
  s.reset()                                                                # two start placements
  d = _push_against_restatement(s, rng, select='last')
  assert d.nb.tolist() == [2.0] * 4 and not bool(d.cpu().speed[:, 2:].any())
  s.step(s.sample())                                                       # the env goes on after an in-place push
  assert s.state()[1].tolist() == [3] * 4
  s.close()
  v2 = envs.make('Stack-v2', n_parallel=4, seed=21, pool=ref_pool, block=True, episode_length=4, orientation_freedom=2, ordering_freedom=True, **KW)
  v2.reset()
  for _ in range(2):
    v2.step(v2.sample())
  d = _push_against_restatement(v2, rng)
  assert d.nb.tolist() == [2.0] * 4
  v2.close()


def test_pipelined_env_equals_the_single_handle(ref_pool):
  from stackrl_amd import env as envs
  L, B = 4, 4
  one = _mk(ref_pool, L, n=B, seed=9)
  pipe = _mk(ref_pool, L, n=B, seed=9, cls=envs.PipelinedVecStackEnv, groups=2)
  one.reset(), pipe.reset()
  a = _centre(one, B)
  rng = np.random.RandomState(8)
  for t in range(2):
    one.step(a), pipe.step(a)
    (p1, n1), (p2, n2) = one.poses(), pipe.poses()
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)) and torch.equal(n1, n2) and n1.tolist() == [t + 1] * B
    assert _same_distances(one.distances(tol=TOL), pipe.distances(tol=TOL))
  dv = _cuda(rng.normal(scale=0.2, size=(B, 3)).astype(F32))
  x, y = one.push(dv, 10, tol=TOL), pipe.push(dv, 10, tol=TOL)
  assert _same_distances(x, y) and float(x.max_perr.min()) > 0
  assert np.array_equal(one.state()[0].view(np.int32), pipe.state()[0].view(np.int32))
  one.kick(dv, 'last'), pipe.kick(dv, 'last')
  assert _same_distances(one.distances(since=(p1, n1), tol=TOL), pipe.distances(since=(p2, n2), tol=TOL))
  _same = [torch.equal(u, v) for u, v in zip(one.step(a)[0], pipe.step(a)[0])]   # both render the pushed piles
  assert all(_same)
  one.close(), pipe.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(ref_pool):
  from stackrl_amd import lib as _lib
  from stackrl_amd.config import EINVAL, OK
  lib = _lib.load()
  L = 4
  g = _mk(ref_pool, L)
  poses = torch.zeros((N, L, 8), dtype=torch.float32, device='cuda')
  nb = torch.zeros(N, dtype=torch.int32, device='cuda')
  rows = torch.zeros((N, L, 4), dtype=torch.float32, device='cuda')
  summary = torch.zeros((N, 8), dtype=torch.float32, device='cuda')
  P = lambda t: t.data_ptr()

  def refused(export, text, *args):
    assert getattr(lib, export)(*args) == EINVAL, (export, args)
    assert text in lib.srl_last_error().decode(), lib.srl_last_error()
  refused('srl_poses', 'null env', None, P(poses), P(nb), None)
  refused('srl_poses', 'null output', g._h, None, P(nb), None)
  refused('srl_poses', 'null output', g._h, P(poses), None, None)
  refused('srl_poses', '16-byte aligned', g._h, P(poses) + 4, P(nb), None)
  refused('srl_kick', 'null env', None, P(poses), 1, -1, None)
  refused('srl_kick', 'null increments', g._h, None, 1, -1, None)
  refused('srl_kick', '16-byte aligned', g._h, P(poses) + 8, 1, -1, None)
  refused('srl_kick', 'per_body must be 0 or 1', g._h, P(poses), 2, -1, None)
  refused('srl_kick', 'per_body must be 0 or 1', g._h, P(poses), -1, -1, None)
  refused('srl_kick', 'select must be', g._h, P(poses), 1, -3, None)
  refused('srl_kick', 'select must be', g._h, P(poses), 1, L, None)
  refused('srl_pose_distances', 'null env', None, None, None, 0.0, 0.0, P(rows), P(summary), None)
  refused('srl_pose_distances', 'null output', g._h, None, None, 0.0, 0.0, None, P(summary), None)
  refused('srl_pose_distances', 'null output', g._h, None, None, 0.0, 0.0, P(rows), None, None)
  refused('srl_pose_distances', '16-byte aligned', g._h, P(poses) + 4, P(nb), 0.0, 0.0, P(rows), P(summary), None)
  torch.cuda.synchronize()
  assert not bool(poses.any()) and not bool(rows.any()) and not bool(summary.any())            # refused before any launch
  g.reset()
  a = _centre(g)
  g.step(a)
  dv = torch.ones((N, 8), device='cuda')
  v0 = g.velocities()
  for bad in (L, 31, -1, 'first', True):
    with pytest.raises(ValueError, match='select must be'):
      g.kick(dv, select=bad)
  for shape in [(N, 4), (N + 1, 8), (N, L + 1, 8), (8,)]:
    with pytest.raises(ValueError, match='dv must have shape'):
      g.kick(torch.ones(shape, device='cuda'))
  with pytest.raises(ValueError, match='since must be'):
    g.distances(since=(poses[:, :, :7], nb))
  assert pc.same_bits(g.velocities(), v0)
  # a kick leaves the staged records stale: no state until the next step
  g.get_state()
  g.kick(dv)
  with pytest.raises(ValueError, match='stale'):
    g.get_state()
  g.step(a)
  g.get_state()
  assert lib.srl_poses(g._h, P(poses), P(nb), None) == OK and lib.srl_pose_distances(g._h, P(poses), P(nb), 0.0, 0.0, P(rows), P(summary), None) == OK
  torch.cuda.synchronize()
  assert nb.tolist() == [2] * N and summary[:, 0].tolist() == [2.0] * N
  g.close()
