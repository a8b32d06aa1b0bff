"""Oracle parity of every launch variant of the settle kernel, at the episode lengths where one variant hands over to the
next, on piles (deep contact graphs) and at the manifold-slot cap.

`srl_load_meshes` picks the variant from episode_length (stackrl_hip.hip): `srl_k_step` up to 8 rocks, `srl_k_step_pp1`
(four waves) or `srl_k_step_t128` (two waves, two points per thread) for 9 - 16, `srl_k_step_pp2` above; every case asserts
the variant that ran (`step_variant()`), so that a misspelt or late-read SRL_STEP_VARIANT cannot quietly test the default.
The bar is bit-exact: observations, rewards, done, poses, velocities, sub-step and sweep counts, contact statistics.
The scripts are tests/settle_scenarios.py's; test_settle_scenarios.py holds their hardness on the CPU oracle."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import settle_scenarios as S
from test_parity_gpu import _cmp_step

pytestmark = pytest.mark.gpu

K_STEP, K_PP1, K_PP2, K_T128 = 0, 1, 2, 3
SHAPE = {K_STEP: (128, 1), K_PP1: (256, 1), K_PP2: (256, 2), K_T128: (128, 2)}   # (threads, points per thread)


def _mk(ref_pool, oracle_mod, n, L, kernel, seed, monkeypatch, **kw):
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  if kernel == K_PP1:
    monkeypatch.setenv('SRL_STEP_VARIANT', 'four_wave')
  elif kernel == K_T128:
    monkeypatch.setenv('SRL_STEP_VARIANT', 'two_wave')
  else:
    monkeypatch.delenv('SRL_STEP_VARIANT', raising=False)
  g = envs.VecStackEnv(n_parallel=n, seed=seed, pool=ref_pool, block=True, episode_length=L, **kw)
  o = oracle_mod.OracleEnv(StackConfig(n_envs=n, episode_length=L, **kw), ref_pool, seed=seed)
  assert g.step_variant() == SHAPE[kernel] + (kernel,), 'L = {}: variant {} ran instead of {}'.format(L, g.step_variant(), kernel)
  return g, o


def _cmp_exact(g, o, envs_, tag):
  """Poses, velocities, sweeps, statuses and contact statistics of `envs_` bit for bit."""
  gp, gnb, gsub, gst = g.state()
  op, onb, osub, ost = o.state()
  e = np.asarray(envs_)
  assert np.array_equal(gnb[e], onb[e]), tag + ': body counts'
  assert np.array_equal(gst[e], ost[e]), tag + ': statuses {} vs {}'.format(gst, ost)
  assert np.array_equal(gsub[e], osub[e]), tag + ': sub-step counts'
  bad = np.argwhere(gp[e] != op[e])
  assert not len(bad), tag + ': poses differ at (env, body, word) {} by up to {}'.format(bad[:4].tolist(), np.abs(gp[e] - op[e]).max())
  gv, ov = g.velocities(), o.velocities()
  bad = np.argwhere(gv[e] != ov[e])
  assert not len(bad), tag + ': velocities differ at {} by up to {}'.format(bad[:4].tolist(), np.abs(gv[e] - ov[e]).max())
  assert np.array_equal(g.sweeps()[e], o.sweeps()[e]), tag + ': sweeps {} vs {}'.format(g.sweeps(), o.sweeps())
  (gm, gn), (om, on) = g.contacts(), o.contacts()
  assert np.array_equal(gn[e], on[e]) and np.array_equal(gm[e], om[e]), tag + ': contacts {} {} vs {} {}'.format(gm, gn, om, on)


CASES = [
  (K_STEP, 1, 6, {}), (K_STEP, 2, 6, {}), (K_STEP, 8, 5, {}),
  (K_PP1, 9, 5, {}), (K_PP1, 12, 5, {}), (K_PP1, 16, 5, {}),          # 12 rocks: 66 pairs over 64 slots
  (K_T128, 9, 5, {}), (K_T128, 12, 5, {}), (K_T128, 16, 5, {}),
  (K_PP2, 17, 4, {}), (K_PP2, 32, 4, {}), (K_PP2, 32, 4, dict(resolution_factor=4)),
]


@pytest.mark.parametrize('kernel,L,n,kw', CASES,
                         ids=['k{}-L{}{}'.format(k, L, '-rf4' if kw else '') for k, L, _, kw in CASES])
def test_pile_episodes_match_the_oracle_bit_for_bit(ref_pool, oracle_mod, monkeypatch, kernel, L, n, kw):
  """A pile episode (rocks dropped on one another at the centre of the map) through `done` and the auto-reset call."""
  g, o = _mk(ref_pool, oracle_mod, n, L, kernel, S.ENV_SEED, monkeypatch, **kw)
  ids, rect, rng = S.pile_script(len(ref_pool), n, L)
  g.set_script(ids, rect); o.set_script(ids, rect)
  gout, oout = g.reset(), o.reset()
  assert np.array_equal(gout[0][0].cpu().numpy(), oout[0][0])
  aw = g.config.overhead_res - g.config.object_res + 1
  for k in range(L + 2):
    a = S.pile_actions(rng, n, aw)
    oout = o.step(a)
    gout = g.step(torch.from_numpy(a).cuda())
    tag = 'L {} call {}'.format(L, k)
    _cmp_step(g, o, gout, oout, tag)
    _cmp_exact(g, o, range(n), tag)
    if k == L - 1:
      assert oout[2].all() and gout[2].all()
    if k == L:
      assert not oout[2].any()
  g.close()


SLOT_CASES = [(K_PP1, 12), (K_T128, 12), (K_PP1, 16), (K_T128, 16), (K_PP2, 32)]


@pytest.mark.parametrize('kernel,L', SLOT_CASES, ids=['k{}-L{}'.format(k, L) for k, L in SLOT_CASES])
def test_slot_cap_full_and_overflowing_envs(ref_pool, oracle_mod, monkeypatch, kernel, L):
  """One batch: env 0 with exactly NS overlapping broadphase pairs (every manifold slot taken), env 1 with NS + 1 (one pair
  finds no slot: SRL_ST_PAIR_OVERFLOW), envs 2 and 3 ordinary piles.  Over `step_simulation` the envs without an overflow
  match the oracle bit for bit, the statuses agree env by env, and the HIP call reports the overflow."""
  n = 4
  NS = 64 if L <= 16 else 128
  g, o = _mk(ref_pool, oracle_mod, n, L, kernel, 5, monkeypatch)
  ids, rect, rng = S.pile_script(len(ref_pool), n, L)
  ids[:2] = np.resize(np.asarray(S.CUBOIDS, np.int32), L)
  g.set_script(ids, rect); o.set_script(ids, rect)
  g.reset(); o.reset()
  aw = g.config.overhead_res - g.config.object_res + 1
  for k in range(L):                     # every rock placed
    a = S.pile_actions(rng, n, aw)
    _cmp_step(g, o, g.step(torch.from_numpy(a).cuda()), o.step(a), 'placing {}'.format(k))
  _cmp_exact(g, o, range(n), 'placed')
  p, v = o.state()[0], o.velocities()
  for e, pairs in ((0, NS), (1, NS + 1)):
    p[e, :L] = S.grid_poses(ref_pool, o.cfg, S.grid_sites(L, pairs))
    p[e, :L, 7] = ids[e]
    v[e] = 0.0
    count, margin = S.box_overlap_pairs(ref_pool, o.cfg, p[e, :L])
    assert count == pairs and margin > 0.05, (count, margin)
  g.set_body_state(p, v); o.set_body_state(p, v)
  for rnd, subs in enumerate((1, 4)):
    o.step_simulation(subs)
    if rnd == 0:
      with pytest.raises(RuntimeError, match='PAIR_OVERFLOW'):
        g.step_simulation(subs)
    else:                                # (the statuses are sticky; whether a pair is left over in these sub-steps is not)
      try:
        g.step_simulation(subs)
      except RuntimeError as err:
        assert 'PAIR_OVERFLOW' in str(err)
    tag = 'L {} step_simulation round {}'.format(L, rnd)
    st = o.state()[3]
    if rnd == 0:                         # the arrangement as built: env 0 exactly full, env 1 one pair over
      assert o.debug_slots(0)[0] == NS and o.debug_slots(1)[0] == NS
      assert list(st & 2) == [0, 2, 0, 0], st
    assert np.array_equal(g.state()[3], st), tag + ': statuses {} vs {}'.format(g.state()[3], st)
    _cmp_exact(g, o, [e for e in range(n) if not st[e] & 2], tag)
  g.close()
