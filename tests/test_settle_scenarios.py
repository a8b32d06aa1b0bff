"""The pile scripts of tests/test_settle_variants_gpu.py stay hard (CPU oracle): rocks dropped at the centre of the map
build contact graphs that random actions do not reach — more manifold slots in use at once than the random-episode maxima
quoted at stackrl_hip.hip nslots (36 at 16 rocks, 85 at 32) and many colours.  The floors sit just below what these
scripts reach today (max over envs and calls of `srlo_debug_slots`), so that a change to the scripts cannot quietly make
the parity cases easy.  Also the slot-cap arrangements: the grid construction gives exactly the pair counts asked for."""
import numpy as np
import pytest

import settle_scenarios as S

# (L, n, kw): the pile cases of test_settle_variants_gpu.py; floors on (active slots, colours)
HARD = [
  (8, 5, {}, 15, 6),            # reached: 16 active slots, 6 colours
  (16, 5, {}, 37, 9),           # 38, 10
  (32, 4, {}, 96, 12),          # 100, 13
  (32, 4, dict(resolution_factor=4), 96, 12),   # 102, 14
]


@pytest.mark.parametrize('L,n,kw,min_active,min_colours', HARD)
def test_pile_scripts_reach_deep_contact_graphs(ref_pool, oracle_mod, L, n, kw, min_active, min_colours):
  from stackrl_amd.config import StackConfig
  cfg = StackConfig(n_envs=n, episode_length=L, **kw)
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=S.ENV_SEED)
  ids, rect, rng = S.pile_script(len(ref_pool), n, L)
  o.set_script(ids, rect)
  o.reset()
  aw = cfg.overhead_res - cfg.object_res + 1
  top = np.zeros(4, np.int64)
  for _ in range(L + 2):
    o.step(S.pile_actions(rng, n, aw))
    assert o.rc == 0
    top = np.maximum(top, np.max([o.debug_slots(i) for i in range(n)], 0))
  active, with_points, points, colours = top
  assert active >= min_active and colours >= min_colours, 'L = {}: at most {} active slots, {} colours'.format(L, active, colours)
  assert with_points > 0 and points >= with_points


@pytest.mark.parametrize('L,ns', [(12, 64), (16, 64), (32, 128)])
def test_slot_cap_arrangements_have_the_pair_counts_asked_for(ref_pool, oracle_mod, L, ns):
  """NS and NS + 1 overlapping broadphase pairs, by the grid rule, by the grown boxes in float64 (a tenth of a box from the
  threshold at least) and by the oracle's broadphase after one sub-step (all NS slots taken; one pair left over)."""
  from stackrl_amd.config import StackConfig
  cfg = StackConfig(n_envs=2, episode_length=L)
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=S.ENV_SEED)
  o.set_script(np.resize(np.asarray(S.CUBOIDS, np.int32), (2, L)), np.array([[40, 40, 64, 64]] * 2, np.int32))
  o.reset()
  aw = cfg.overhead_res - cfg.object_res + 1
  for _ in range(L):
    o.step(np.full(2, (aw // 2) * aw + aw // 2, np.int64))
  p = o.state()[0]
  for e, pairs in ((0, ns), (1, ns + 1)):
    sites = S.grid_sites(L, pairs)
    assert len(set(sites)) == L and S.overlap_pairs(sites) == pairs
    p[e, :L] = S.grid_poses(ref_pool, cfg, sites)
    count, margin = S.box_overlap_pairs(ref_pool, cfg, p[e, :L])
    assert count == pairs and margin > 0.05
  o.set_body_state(p, np.zeros_like(p))
  o.step_simulation(1)
  assert o.debug_slots(0)[0] == ns and o.debug_slots(1)[0] == ns
  assert list(o.state()[3] & 2) == [0, 2]
