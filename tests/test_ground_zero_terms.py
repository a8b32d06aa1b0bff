"""The exact-zero scenarios of tests/ground_zero_scenarios.py, held on the CPU oracle: that they are what they are for.

tests/test_ground_zero_terms_gpu.py runs them on every settle kernel against the oracle; if a scenario stopped producing
ground and pair points, exact zeros that live through a solved sub-step and a -0 target, that comparison would prove nothing
about the terms the kernels leave out.  The figures here are floors on the scenarios, not tolerances."""
import numpy as np
import pytest

import ground_zero_scenarios as Z

L = 8


@pytest.fixture(scope='module')
def history(ref_pool, oracle_mod):
  """(config, poses and velocities as set, run(): the state after each of SUBSTEPS sub-steps, pair points per sub-step and env)."""
  from stackrl_amd.config import StackConfig
  cfg = StackConfig(n_envs=Z.N_ENVS, episode_length=L, **Z.CFG)
  o = oracle_mod.OracleEnv(cfg, ref_pool, seed=7)
  p, v = Z.place([o], ref_pool, o.cfg, L)
  hist, pair_points = [], []
  for _ in range(Z.SUBSTEPS):
    hist += Z.run(o, 1)
    pair_points.append([o.debug_slots(e)[2] for e in range(Z.N_ENVS)])
  return cfg, p, v, hist, np.asarray(pair_points)


def test_no_env_fails_and_every_cuboid_meets_the_ground(history):
  cfg, p, v, hist, pair_points = history
  for k, (poses, vel, sub, sweeps, st, (max_pen, n_points)) in enumerate(hist):
    assert not st.any(), (k, st)
    assert np.isfinite(vel).all() and np.isfinite(poses).all()
  ground0 = hist[0][5][1] - pair_points[0]
  print('ground points on the first sub-step', ground0, 'pair points', pair_points[0], 'sweeps', hist[0][3])
  assert list(ground0) == [4 * L, 4 * (L - 1), 4 * L, 4 * L, 4 * (L - 1), 4 * L]     # (the upper cuboid of a stack has none)
  assert pair_points[0][Z.STACK] == 4 and pair_points[0][Z.HOVER] == 4                # a full manifold between the flat faces
  assert (pair_points[:, Z.STACK] > 0).all()


def test_target_of_minus_zero_with_zero_relative_velocity(history):
  """TARGET0: dist + linear_slop == 0 — the deepest penetration the oracle reports is linear_slop to the bit, so the normal
  rows' target is -((0 * erp) / dt) = -0 — and gravity cancels the speed set: vrel = 0 in every row, every impulse a zero,
  and after the solved sub-step (4 L ground points) every velocity component is still an exact zero."""
  cfg, p, v, hist, pair_points = history
  poses, vel, sub, sweeps, st, (max_pen, n_points) = hist[0]
  assert max_pen[Z.TARGET0] == np.float32(cfg.linear_slop) and np.float32(cfg.linear_slop) > 0
  assert n_points[Z.TARGET0] == 4 * L and sweeps[Z.TARGET0] >= 1
  assert v[Z.TARGET0, :L, 2].all()                                                   # (a speed was set ...)
  assert not vel[Z.TARGET0].any()                                                    # (... and nothing is left of it)
  assert np.array_equal(poses[Z.TARGET0, :L, :7], p[Z.TARGET0, :L, :7])
  assert hist[1][1][Z.TARGET0, :L, 2].all()                                          # the next sub-step's gravity is met by the ground


def test_exact_zero_components_survive_a_solved_sub_step(history):
  """HOVER: ground points under every cuboid but the upper one, a full pair manifold, and after the first sub-step's solve
  the zero components are zeros still: the lateral speeds set are the only non-zero words (friction bounds -0, +0)."""
  cfg, p, v, hist, pair_points = history
  poses, vel, sub, sweeps, st, (max_pen, n_points) = hist[0]
  assert n_points[Z.HOVER] == 4 * (L - 1) + 4 and sweeps[Z.HOVER] >= 1
  want = np.zeros_like(vel[Z.HOVER])
  want[2, 0], want[3, 1] = vel[Z.HOVER, 2, 0], vel[Z.HOVER, 3, 1]
  assert 0.04 < want[2, 0] < 0.05 and -0.05 < want[3, 1] < -0.04                     # (damped, not stopped: no friction yet)
  assert np.array_equal(vel[Z.HOVER], want)
  # from the second sub-step on the cuboids land: impulses, more than one sweep, and the stack's pair rows at work
  assert hist[1][3][Z.HOVER] > 1 and hist[1][1][Z.HOVER, :L].any(axis=1).all()
  assert (pair_points[:, Z.HOVER] > 0).all()


def test_pressed_cuboids_are_pushed_out_from_zero_velocities(history):
  """FALL, STACK, SLIDE, REST: every velocity component but the ones set starts as an exact zero, and the first sub-step's
  normal rows push (sweeps beyond the first, every cuboid moving up afterwards); SLIDE's friction rows brake the lateral speed."""
  cfg, p, v, hist, pair_points = history
  poses, vel, sub, sweeps, st, (max_pen, n_points) = hist[0]
  for e in (Z.FALL, Z.STACK, Z.SLIDE, Z.REST):
    assert np.count_nonzero(v[e]) <= 2
    assert sweeps[e] > 1 and max_pen[e] > 0.0004
    assert (vel[e, :L, 2] > 0).all(), (e, vel[e, :L, 2])
  assert 0 < vel[Z.SLIDE, 0, 0] < 0.03 and -0.03 < vel[Z.SLIDE, 1, 1] < 0
