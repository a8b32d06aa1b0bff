"""GPU tests of env states as values (csrc/state.hip, stackrl_amd/state.py, stackrl_amd/lookahead.py): a state taken with
`get_state` and put back with `set_state` — into the same env, another slot, another handle, after a trip through a file —
continues bit for bit.  Every comparison is exact: against the CPU oracle where it runs the configuration (with the
comparison of tests/test_parity_gpu.py), run against run elsewhere."""
import ctypes
import io

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

POSE_ATOL = 1e-6


def _mk(ref_pool, oracle_mod, n, L, seed=11, **kw):
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  g = envs.VecStackEnv(n_parallel=n, seed=seed, pool=ref_pool, block=True, episode_length=L, **kw)
  o = oracle_mod.OracleEnv(StackConfig(n_envs=n, episode_length=L, **kw), ref_pool, seed=seed)
  return g, o


def _cmp_step(g, o, gout, oout, tag):
  (gm, go), gr, gd = gout
  (om, oo), orr, od = oout
  assert np.array_equal(gm.cpu().numpy(), om), tag + ': obs_map differs'
  assert np.array_equal(go.cpu().numpy(), oo), tag + ': obs_obj differs'
  assert np.array_equal(gd.cpu().numpy(), od), tag + ': done differs'
  np.testing.assert_allclose(gr.cpu().numpy(), orr, rtol=0, atol=1e-7, err_msg=tag + ': reward')
  gp, gnb, gsub, gst = g.state()
  op, onb, osub, ost = o.state()
  assert np.array_equal(gnb, onb), tag
  assert np.array_equal(gsub, osub), tag + ': sub-step counts differ {} vs {}'.format(gsub[:4], osub[:4])
  assert np.array_equal(gst, ost), tag
  np.testing.assert_allclose(gp, op, rtol=0, atol=POSE_ATOL, err_msg=tag + ': poses')
  gH, gO, gg = g.maps()
  oH, oO, og = o.maps()
  assert np.array_equal(gg, og), tag + ': goal rect'
  np.testing.assert_allclose(gH, oH, rtol=0, atol=1.2e-4, err_msg=tag + ': height map')
  np.testing.assert_allclose(gO, oO, rtol=0, atol=1.2e-4, err_msg=tag + ': object map')


def _script(g, o, ref_pool, n, L, rng):
  ids = np.stack([rng.choice(len(ref_pool), size=L, replace=False) for _ in range(n)]).astype(np.int32)
  H = g.config.overhead_res
  rect = np.stack([[rng.randint(H // 16, H // 4), rng.randint(H // 16, H // 4), H // 2, H // 2] for _ in range(n)]).astype(np.int32)
  g.set_script(ids, rect)
  if o is not None:
    o.set_script(ids, rect)


def _same(a, b, tag=''):
  """Two step tuples, bit for bit."""
  (am, ao), ar, ad = a
  (bm, bo), br, bd = b
  assert am.dtype == bm.dtype and torch.equal(am, bm), tag + ': obs_map differs'
  assert torch.equal(ao, bo), tag + ': obs_obj differs'
  assert torch.equal(ar.view(torch.int32), br.view(torch.int32)), tag + ': reward differs'
  assert torch.equal(ad, bd), tag + ': done differs'


def _cuda(a):
  return torch.from_numpy(np.asarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. detour against the oracle
@pytest.mark.parametrize('L,n,kw', [
  (8, 6, {}),
  (5, 7, dict(resolution_factor=3)),       # a 32 x 32 map: the record is smaller than one pass of the copy's workgroups
  (12, 6, dict(resolution_factor=4)),
  (32, 3, dict(resolution_factor=4)),      # the `pp2` settle variant and the largest blob
  (6, 4, dict(rewarder='all')),            # four reward memories
])
def test_detour_and_restore_continues_like_the_oracle(ref_pool, oracle_mod, L, n, kw):
  g, o = _mk(ref_pool, oracle_mod, n, L, **kw)
  rng = np.random.RandomState(5)
  _script(g, o, ref_pool, n, L, rng)
  g.reset(), o.reset()
  A = g.n_actions
  acts = rng.randint(0, A, size=(L + 2, n)).astype(np.int64)
  other = rng.randint(0, A, size=(2, n)).astype(np.int64)
  for k in range(L + 2):                   # through done and the auto-reset step
    if k == 3:
      at3 = gout
      snap = g.get_state()
      assert tuple(snap.records.shape) == (n, g.get_state().records.shape[1]) and snap.left == L - 3
      for a in other:
        g.step(_cuda(a))
      back = g.set_state(snap)
      _same(back, at3, 'the stored step')
      assert torch.equal(g.get_state().records, snap.records)
    gout = g.step(_cuda(acts[k]))
    _cmp_step(g, o, gout, o.step(acts[k]), 'step {}'.format(k))
  g.close()


# ------------------------------------------------------------------------------------------------ 2. across the reset
def test_restore_brings_the_episode_and_sample_counters_back(ref_pool):
  from stackrl_amd import env as envs
  n, L = 8, 4
  g = envs.VecStackEnv(n_parallel=n, seed=123, pool=ref_pool, block=True, episode_length=L)
  g.reset()
  for _ in range(2):
    g.step(g.sample())
  snap = g.get_state()

  def run():
    log = []
    for _ in range(2, 2 * L + 3):
      a = g.sample()
      log.append((a.clone(), g.step(a)))
    return log
  first = run()
  assert sum(int(out[2].any()) for _, out in first) == 2                      # two episodes end on the way
  g.set_state(snap)
  for t, ((a1, out1), (a2, out2)) in enumerate(zip(first, run())):
    assert torch.equal(a1, a2), 'sampled actions differ at step {}'.format(t)
    _same(out1, out2, 'step {}'.format(t))
  g.close()


# ------------------------------------------------------------------------------------------------ 3. fork equals restore
def test_lookahead_of_each_candidate_equals_restore_and_step(ref_pool, oracle_mod):
  from stackrl_amd.lookahead import Lookahead
  n, L, k = 4, 8, 3
  g, o = _mk(ref_pool, oracle_mod, n, L)
  rng = np.random.RandomState(8)
  _script(g, o, ref_pool, n, L, rng)
  g.reset(), o.reset()
  A = g.n_actions
  for t in range(3):
    a = rng.randint(0, A, size=n).astype(np.int64)
    _cmp_step(g, o, g.step(_cuda(a)), o.step(a), 'step {}'.format(t))
  look = Lookahead(g, k)
  assert look.scratch.batch_size == n * k
  snap = g.get_state()
  cand = _cuda(rng.randint(0, A, size=(n, k)).astype(np.int64))
  (om, oo), r, d = look.evaluate(cand, observations=True)
  assert tuple(r.shape) == (n, k) and tuple(om.shape[:2]) == (n, k)
  assert torch.equal(g.get_state().records, snap.records)                       # the env itself was not touched:
  a = rng.randint(0, A, size=n).astype(np.int64)
  _cmp_step(g, o, g.step(_cuda(a)), o.step(a), 'the step after evaluate')       # its next step is the oracle's
  for j in range(k):
    g.set_state(snap)
    _same(g.step(cand[:, j]), ((om[:, j], oo[:, j]), r[:, j], d[:, j]), 'candidate {}'.format(j))
  look.close(); g.close()


# ------------------------------------------------------------------------------------------------ 4. across settle variants
def test_fork_into_the_two_wave_variant_equals_the_oracle(ref_pool, oracle_mod, monkeypatch):
  from stackrl_amd.lookahead import Lookahead
  L, n = 14, 5
  monkeypatch.setenv('SRL_STEP_VARIANT', 'four_wave')
  g, o = _mk(ref_pool, oracle_mod, n, L, seed=17)
  monkeypatch.setenv('SRL_STEP_VARIANT', 'two_wave')       # read at srl_create: the scratch handle's
  look = Lookahead(g, 1)
  assert g.step_variant() == (256, 1, 1) and look.scratch.step_variant() == (128, 2, 3)
  g.reset(), o.reset()
  for t in range(L - 1):
    ga, oa = g.sample(), o.sample()
    assert np.array_equal(ga.cpu().numpy(), oa)
    if t in (5, L - 2):                                    # a production batch of 3,072 envs or more steps the two-wave kernel
      obs, r, d = look.evaluate(ga[:, None], observations=True)
    gout, oout = g.step(ga), o.step(oa)
    _cmp_step(g, o, gout, oout, 'step {}'.format(t))
    if t in (5, L - 2):
      _same(((obs[0][:, 0], obs[1][:, 0]), r[:, 0], d[:, 0]), gout, 'forked step {}'.format(t))
  look.close(); g.close()


# ------------------------------------------------------------------------------------------------ 5. partial set
def test_partial_set_writes_the_named_envs_only(ref_pool):
  from stackrl_amd import env as envs
  n, L = 6, 6
  g = envs.VecStackEnv(n_parallel=n, seed=3, pool=ref_pool, block=True, episode_length=L)
  g.reset()
  for _ in range(2):
    g.step(g.sample())
  before = g.get_state()
  part = g.get_state([1, 4])
  assert torch.equal(part.records, before.records[[1, 4]]) and torch.equal(part.obs[0], before.obs[0][[1, 4]])
  back = g.set_state(part, indexes=[0, 5])
  _same(back, before.step_tuple([1, 4]), 'the stored step')
  after = g.get_state()
  assert torch.equal(after.records[1:5], before.records[1:5])                   # word for word
  assert torch.equal(after.records[[0, 5]], before.records[[1, 4]])
  assert not torch.equal(before.records[0], before.records[1])
  a = g.sample()
  a[0], a[5] = a[1], a[4]
  (om, oo), r, d = g.step(a)
  for dst, src in ((0, 1), (5, 4)):
    assert torch.equal(om[dst], om[src]) and torch.equal(oo[dst], oo[src]) and float(r[dst]) == float(r[src]) and bool(d[dst]) == bool(d[src])
  assert not torch.equal(om[0], om[2])
  # the checks of the Python side and of the export
  with pytest.raises(ValueError, match='distinct'):
    g.set_state(part, indexes=[2, 2])
  stale = g.get_state([1, 4])
  g.step(g.sample())
  with pytest.raises(ValueError, match='point of the episode'):
    g.set_state(stale, indexes=[0, 5])
  L_ = g._lib
  rec = before.records.clone()
  own = g.state_signature()
  now = g.get_state().records
  assert L_.srl_state_set(g._h, ctypes.c_uint64(own ^ 1), None, None, n, rec.data_ptr(), None) == 1       # refused before any launch
  from stackrl_amd import lib
  assert lib.last_error().startswith("srl_state_set: the records' signature is not this handle's")
  assert torch.equal(g.get_state().records, now)
  g.step_simulation(1)                                     # a test hook moved bodies: the staged records are stale
  with pytest.raises(ValueError, match='stale'):
    g.get_state()
  g.close()


# ------------------------------------------------------------------------------------------------ 6. Stack-v2 and the wrappers
def test_detour_on_stack_v2_with_both_freedoms(ref_pool, oracle_mod):
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  n, L, k = 4, 4, 2
  g = envs.make('Stack-v2', n_parallel=n, seed=21, pool=ref_pool, block=True, episode_length=L, orientation_freedom=k, ordering_freedom=True)
  o = oracle_mod.OracleEnv(StackConfig(n_envs=n, episode_length=L, orientation_freedom=k, ordering_freedom=True), ref_pool, seed=21)
  g.reset(), o.reset()
  for t in range(2 * (L + 1)):
    if t == 2:
      snap = g.get_state()
      shown = g.num_maps_on_show
      for _ in range(2):
        g.step(g.sample())                                 # (also moves the sample counter on)
      g.set_state(snap)
      assert g.num_maps_on_show == shown
    a = g.sample()
    assert np.array_equal(a.cpu().numpy(), o.sample())
    (gm, go), gr, gd = g.step(a)
    (om, oo), orr, od = o.step(a.cpu().numpy())
    assert np.array_equal(gm.cpu().numpy(), om) and np.array_equal(go.cpu().numpy(), oo), t
    assert np.array_equal(gd.cpu().numpy().astype(bool), od) and np.array_equal(gr.cpu().numpy(), orr), t
    assert np.array_equal(g.state()[0], o.state()[0]) and np.array_equal(g.maps()[1], o.maps()[1]), t
  g.close()


def _run_against_run(make, steps, snap_at, seed=0):
  """Two envs from `make()` on the same actions; the second takes a snapshot before step `snap_at`, two steps with other
  actions, and restores: every step of the two is the same."""
  a, b = make(), make()
  gen = torch.Generator().manual_seed(seed)
  _same(a.reset(), b.reset(), 'reset')
  last = None
  for t in range(steps):
    act = torch.randint(0, a.n_actions, (a.batch_size,), generator=gen).cuda()
    if t == snap_at:
      snap = b.get_state()
      for _ in range(2):
        b.step(torch.randint(0, a.n_actions, (a.batch_size,), generator=gen).cuda())
      _same(b.set_state(snap), last, 'the stored step')
    last = a.step(act)
    _same(last, b.step(act), 'step {}'.format(t))
  return a, b


def test_detour_on_a_pipelined_env_equals_one_handle(ref_pool):
  from stackrl_amd import env as envs
  n, L = 6, 4
  pipe = envs.PipelinedVecStackEnv(n_parallel=n, groups=2, seed=9, pool=ref_pool, block=True, episode_length=L)
  one = envs.VecStackEnv(n_parallel=n, seed=9, pool=ref_pool, block=True, episode_length=L)
  envs_ = iter((one, pipe))
  _run_against_run(lambda: next(envs_), 2 * L, 2)
  s = pipe.get_state([4, 1])                               # across the groups, in the order asked for
  own = [pipe._envs[1].get_state([1]), pipe._envs[0].get_state([1])]      # (words no step has written yet differ between handles)
  assert torch.equal(s.records, torch.cat([p.records for p in own]))
  assert torch.equal(s.obs[0], one.get_state().obs[0][[4, 1]]) and s.left == one.get_state().left
  pipe.close(); one.close()


@pytest.mark.parametrize('kw', [dict(), dict(min_episode_length=1), dict(dtype='float32', start_policy=lambda obs: torch.full((4,), 1234, dtype=torch.int64, device='cuda'))])
def test_detour_on_a_started_env_and_on_float32_observations(ref_pool, kw):
  from stackrl_amd import env as envs
  a, b = _run_against_run(lambda: envs.StartedVecStackEnv(n_parallel=4, n_objects=6, episode_length=3, seed=5, pool=ref_pool, block=True, **kw), 9, 2)
  assert a._last[0][0].dtype == (torch.float32 if 'dtype' in kw else torch.uint8)
  a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 7. host round trip
def test_state_survives_a_file_and_a_fresh_env(ref_pool):
  from stackrl_amd import env as envs
  from stackrl_amd.state import EnvState
  n, L = 4, 5
  g = envs.VecStackEnv(n_parallel=n, seed=11, pool=ref_pool, block=True, episode_length=L)
  g.reset()
  for _ in range(3):
    last = g.step(g.sample())
  buf = io.BytesIO()
  torch.save(g.get_state().cpu().state_dict(), buf)
  buf.seek(0)
  state = EnvState.from_state_dict(torch.load(buf, weights_only=True)).to('cuda')
  h = envs.VecStackEnv(n_parallel=n, seed=77, pool=ref_pool, block=True, episode_length=L)      # fresh: never reset, another seed
  _same(h.set_state(state), last, 'the stored step')
  for t in range(L + 2):                                   # through the auto-reset: the seed and the counters came along
    a, b = g.sample(), h.sample()
    assert torch.equal(a, b)
    _same(g.step(a), h.step(b), 'step {}'.format(t))
  longer = envs.VecStackEnv(n_parallel=n, seed=11, pool=ref_pool, block=True, episode_length=L + 1)
  other = envs.VecStackEnv(n_parallel=n, seed=11, pool=ref_pool.subset(list(range(len(ref_pool) - 1))), block=True, episode_length=L)
  for e in (longer, other):
    with pytest.raises(ValueError, match='signature'):
      e.set_state(state)
    e.close()
  g.close(); h.close()


# ------------------------------------------------------------------------------------------------ 8. LookaheadPolicy
def test_lookahead_policy_predicts_the_reward_it_then_gets(ref_pool):
  from stackrl_amd import env as envs
  from stackrl_amd.baselines import Baseline
  from stackrl_amd.lookahead import Lookahead, LookaheadPolicy
  n, L = 4, 6
  g = envs.VecStackEnv(n_parallel=n, seed=2, pool=ref_pool, block=True, episode_length=L)
  base = Baseline('height', value=True)
  one, four = LookaheadPolicy(base, Lookahead(g, 1)), LookaheadPolicy(base, Lookahead(g, 4))
  obs = g.reset()[0]
  for t in range(L):
    a0, v0 = base(obs)
    a1, v1 = one(obs)
    assert torch.equal(a0.to(torch.int64), a1) and torch.equal(v0, v1)          # k = 1 is the base policy
    a4, _ = four(obs)
    cand, pred = four.last
    assert torch.equal(cand[:, 0], a0.to(torch.int64))
    obs, r, d = g.step(a4)
    rank = (cand == a4[:, None]).to(torch.int8).argmax(1)
    chosen = pred.gather(1, rank[:, None])[:, 0]
    assert torch.equal(r.view(torch.int32), chosen.view(torch.int32)), 'step {}: the reward is not the predicted one'.format(t)
    assert bool((r >= pred[:, 0]).all())
  assert bool(d.all())
  with pytest.raises(ValueError, match='auto-reset'):
    four.lookahead.evaluate(cand)
  for p in (one, four):
    p.lookahead.close()
  g.close()
