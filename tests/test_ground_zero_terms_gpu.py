"""Every settle kernel against the oracle where the solver's rows meet exact zeros, and on random rocks at the smallest shapes
that reach each form of the ground points' records.

The kernels evaluate a ground row without the product with its structural zero, from records that share the four distinct
ca words of a point, and form a friction row's impulse as a plain product instead of an FMA onto 0 * rk
(stackrl_amd/csrc/solver.h, "The rows' structural zeros"); the oracle states the full expressions.  The argument there says that
only the sign of an exact zero can differ, and only in a velocity or an accumulated impulse that is a zero on both sides.
The scenarios of tests/ground_zero_scenarios.py are built to reach those zeros (tests/test_ground_zero_terms.py holds on the
CPU that they do); the random rocks of the parity suite never do.

No call returns the accumulated impulses, on either side.  They are compared through what they do: each sub-step warm-starts
from the impulses the last one left, so a difference in value shows in the next sub-step's velocities and sweep count."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import ground_zero_scenarios as Z
from test_parity_gpu import _cmp_step
from test_settle_variants_gpu import K_PP1, K_PP2, K_STEP, K_T128, SHAPE, _cmp_exact, _mk

pytestmark = pytest.mark.gpu

# (kernel, rocks): the fewest rocks each kernel runs at (srl_k_step: the most, where the body lanes are all in use)
KERNELS = [(K_STEP, 8), (K_PP1, 9), (K_T128, 9), (K_PP2, 17)]


@pytest.mark.parametrize('kernel,L', KERNELS, ids=['k{}-L{}'.format(k, L) for k, L in KERNELS])
def test_exact_zero_scenarios_match_the_oracle(ref_pool, oracle_mod, monkeypatch, kernel, L):
  g, o = _mk(ref_pool, oracle_mod, Z.N_ENVS, L, kernel, 7, monkeypatch, **Z.CFG)
  p, v = Z.place([g, o], ref_pool, o.cfg, L)
  assert np.array_equal(g.state()[0].view(np.uint32), o.state()[0].view(np.uint32))
  for k in range(Z.SUBSTEPS):
    (gp, gv, gsub, gsw, gst, (gmp, gn)), = Z.run(g, 1)
    (op, ov, osub, osw, ost, (omp, on)), = Z.run(o, 1)
    tag = 'kernel {} sub-step {}'.format(kernel, k)
    assert not ost.any() and np.array_equal(gst, ost), tag + ': statuses {} vs {}'.format(gst, ost)
    # poses bit for bit
    bad = np.argwhere(gp.view(np.uint32) != op.view(np.uint32))
    assert not len(bad), tag + ': poses differ at (env, body, word) {}'.format(bad[:4].tolist())
    # velocities by value: the sign of an exact zero is the one thing that may differ (0.0 == -0.0)
    bad = np.argwhere(gv != ov)
    assert not len(bad), tag + ': velocities differ at {} by up to {}'.format(bad[:4].tolist(), np.abs(gv - ov).max())
    assert np.array_equal(gsub, osub), tag + ': sub-step counts'
    assert np.array_equal(gsw, osw), tag + ': sweeps {} vs {}'.format(gsw, osw)
    assert np.array_equal(gn, on) and np.array_equal(gmp, omp), tag + ': contacts {} {} vs {} {}'.format(gmp, gn, omp, on)
    if k == 0:      # the scenarios are in place on this handle too (tests/test_ground_zero_terms.py: what the oracle does with them)
      assert not gv[Z.TARGET0].any() and gmp[Z.TARGET0] == np.float32(o.cfg.linear_slop)
      assert np.count_nonzero(gv[Z.HOVER]) == 2
  g.close()


# the smallest shapes that reach each form of the records: 8 rocks (srl_k_step: records requested a point ahead, and the
# ground-only sweeps from registers), 9 (srl_k_step_pp1: point lanes, no records), 16 told that 4,096 envs share the device
# (srl_k_step_t128: records read as needed), 17 (srl_k_step_pp2: the same with two points per thread)
SHAPES = [(K_STEP, 8, {}), (K_PP1, 9, {}), (K_T128, 16, dict(concurrent_envs=4096)), (K_PP2, 17, {})]


@pytest.mark.parametrize('kernel,L,kw', SHAPES, ids=['k{}-L{}'.format(k, L) for k, L, _ in SHAPES])
def test_random_rock_episode_matches_the_oracle_bit_for_bit(ref_pool, oracle_mod, kernel, L, kw):
  """One episode of random rocks and actions, 8 envs, through `done`."""
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  n = 8
  g = envs.VecStackEnv(n_parallel=n, seed=23, pool=ref_pool, block=True, episode_length=L, **kw)
  o = oracle_mod.OracleEnv(StackConfig(n_envs=n, episode_length=L), ref_pool, seed=23)
  assert g.step_variant() == SHAPE[kernel] + (kernel,)
  gout, oout = g.reset(), o.reset()
  assert np.array_equal(gout[0][0].cpu().numpy(), oout[0][0]) and np.array_equal(gout[0][1].cpu().numpy(), oout[0][1])
  for k in range(L):
    ga, oa = g.sample(), o.sample()
    assert np.array_equal(ga.cpu().numpy(), oa)
    gout, oout = g.step(ga), o.step(oa)
    _cmp_step(g, o, gout, oout, 'step {}'.format(k))
    _cmp_exact(g, o, range(n), 'step {}'.format(k))
  assert oout[2].all() and gout[2].all()
  g.close()
