"""Arrangements that take `srl_k_step`'s pair solver where the pile scripts never go, held on the CPU oracle.

The pile scripts at 8 rocks put at most 11 point-bearing manifold slots into an env, about two points each: every point sits
in wave 0 (slots 0 - 15), the sweeps are solo, and the turns of a manifold's third and fourth point may never run.  Eight
cuboids on the grid of tests/settle_scenarios.py with 24 or 28 overlapping pairs put points into slots past the sixteenth (a
pair point in wave 1: sweeps with block barriers); with 17 pairs the run ends with every point-bearing manifold full (four
points: both lane pairs of a slot's quad take both their turns).  tests/test_pair_split_gpu.py runs the same arrangements on
the GPU; this file keeps them what they are.  The figures are floors on the scenario, not tolerances."""
import numpy as np
import pytest

import settle_scenarios as S

L = 8
SUBSTEPS = 60
ARRANGEMENTS = (24, 28, 17)      # overlapping broadphase pairs of env 0, 1, 2 (`arrange`)


def arrange(envs_, ref_pool, cfg, pairs=ARRANGEMENTS, x0=None):
  """Every handle of `envs_` (the same shape, oracle or GPU) with 8 cuboids placed, then laid out at rest on the grid: env e
  with pairs[e] overlapping pairs, its grid's corner at x0[e] (default: the origin).  Returns the poses set."""
  n = cfg.n_envs
  ids = np.tile(np.resize(np.asarray(S.CUBOIDS, np.int32), L), (n, 1))      # every env the same three masses in turn
  rect = np.array([[40, 40, 64, 64]] * n, np.int32)
  aw = cfg.overhead_res - cfg.object_res + 1
  a = np.full(n, (aw // 2) * aw + aw // 2, np.int64)
  for h in envs_:
    h.set_script(ids, rect)
    h.reset()
  for _ in range(L):
    for h in envs_:
      h.step(a if not hasattr(h, 'step_variant') else _device(a))
  p = np.array(envs_[0].state()[0], np.float32)
  for e in range(n):
    want = pairs[e]
    p[e, :L] = S.grid_poses(ref_pool, cfg, S.grid_sites(L, want), x0=(0.0, 0.0) if x0 is None else x0[e])
    p[e, :L, 7] = ids[e]
    count, margin = S.box_overlap_pairs(ref_pool, cfg, p[e, :L])
    assert count == want and margin > 0.05, (count, margin)
  v = np.zeros_like(p)
  for h in envs_:
    h.set_body_state(p, v)
  return p


def _device(a):
  import torch
  return torch.from_numpy(a).cuda()


@pytest.fixture(scope='module')
def slot_history(ref_pool, oracle_mod):
  """`debug_slots` of the three arrangements after each of 60 sub-steps: [sub-step][env] = (active, with points, points, colours)."""
  from stackrl_amd.config import StackConfig
  cfg = StackConfig(n_envs=len(ARRANGEMENTS), episode_length=L)
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=S.ENV_SEED)
  arrange([o], ref_pool, cfg)
  hist = []
  for _ in range(SUBSTEPS):
    o.step_simulation(1)
    hist.append([o.debug_slots(e) for e in range(cfg.n_envs)])
  assert not o.state()[3].any(), o.state()[3]
  return np.asarray(hist)


@pytest.mark.parametrize('env', [0, 1], ids=['pairs24', 'pairs28'])
def test_points_reach_slots_past_the_sixteenth(slot_history, env):
  """>= 17 slots with contact points in some sub-step: a slot index >= 16 holds points, so wave 1 holds a pair point and the
  sweeps of that sub-step are not solo.  (On the oracle: 5 and 7 of the 60 sub-steps; the first sub-step (24, 24, 24, 8) and
  (28, 28, 28, 9).)"""
  with_points = slot_history[:, env, 1]
  print('pairs {}: sub-steps with >= 17 point-bearing slots: {}; first sub-step {}'.format(
    ARRANGEMENTS[env], int((with_points >= 17).sum()), tuple(slot_history[0, env])))
  assert (with_points >= 17).any()
  assert with_points.max() <= 28     # NS of the 8-rock variant: no overflow in these arrangements


def test_manifolds_end_full(slot_history):
  """17 pairs: after 60 sub-steps every point-bearing manifold holds four points (on the oracle: (7, 4, 16, 3))."""
  active, with_points, points, colours = slot_history[-1, 2]
  print('pairs 17 after {} sub-steps: {}'.format(SUBSTEPS, tuple(slot_history[-1, 2])))
  assert with_points > 0 and points == 4 * with_points
