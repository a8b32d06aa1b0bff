"""`srl_k_step`'s pair solver — a contact solved on two lanes, one per body (settle.hip: pair_phase) — against the oracle, bit
for bit, where the pile scripts do not take it: pair points in wave 1 (sweeps with block barriers) and full manifolds (both
lane pairs of a slot's quad take both their turns).  The arrangements are tests/test_pair_split_scenarios.py's, which holds on
the CPU oracle that they stay what they are."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import settle_scenarios as S
import test_pair_split_scenarios as A
from test_parity_gpu import _cmp_step
from test_settle_variants_gpu import K_STEP, _cmp_exact, _mk

pytestmark = pytest.mark.gpu

N = 2


@pytest.mark.parametrize('pairs', A.ARRANGEMENTS, ids=['pairs{}'.format(p) for p in A.ARRANGEMENTS])
def test_grid_arrangements_match_the_oracle_bit_for_bit(ref_pool, oracle_mod, monkeypatch, pairs):
  """Two envs with the arrangement (the second a few centimetres aside, so that it is no copy of the first), 60 sub-steps;
  poses, velocities, sweeps, statuses and contacts after each of the first 10 and after every tenth."""
  g, o = _mk(ref_pool, oracle_mod, N, A.L, K_STEP, S.ENV_SEED, monkeypatch)
  A.arrange([g, o], ref_pool, o.cfg, pairs=(pairs,) * N, x0=((0.0, 0.0), (0.03, 0.02)))
  _cmp_exact(g, o, range(N), 'pairs {} as placed'.format(pairs))
  seen = 0
  for k in range(1, A.SUBSTEPS + 1):
    g.step_simulation(1); o.step_simulation(1)
    seen = max(seen, o.debug_slots(0)[1])
    if k <= 10 or k % 10 == 0:
      _cmp_exact(g, o, range(N), 'pairs {} sub-step {}'.format(pairs, k))
  if pairs != 17:
    assert seen >= 17, seen          # (the CPU file's floor: the barrier path ran with pair points)
  g.close()


def test_pile_episode_through_done_and_reset(ref_pool, oracle_mod, monkeypatch):
  """One pile episode at 8 rocks, five envs, through `done` and the auto-reset call."""
  n = 5
  g, o = _mk(ref_pool, oracle_mod, n, A.L, K_STEP, S.ENV_SEED, monkeypatch)
  ids, rect, rng = S.pile_script(len(ref_pool), n, A.L)
  g.set_script(ids, rect); o.set_script(ids, rect)
  gout, oout = g.reset(), o.reset()
  assert np.array_equal(gout[0][0].cpu().numpy(), oout[0][0])
  aw = g.config.overhead_res - g.config.object_res + 1
  for k in range(A.L + 2):
    a = S.pile_actions(rng, n, aw)
    oout = o.step(a)
    gout = g.step(torch.from_numpy(a).cuda())
    _cmp_step(g, o, gout, oout, 'call {}'.format(k))
    _cmp_exact(g, o, range(n), 'call {}'.format(k))
    if k == A.L - 1:
      assert oout[2].all() and gout[2].all()
  g.close()
