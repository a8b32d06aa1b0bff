"""Oracle parity of the env kernels across `srl_config`, not only at its defaults: the cases of tests/config_cases.py —
solver and physics parameters one at a time (the `bullet10` preset, sweep caps that every sub-step runs into, warm start,
slop, erp, margin, friction, damping, gravity, rest threshold, time step, rock size, `place_at_com = False`), the same on
the other launch variants of the settle kernel, Stack-v2 placements by the link frame, the reward exponents, and goal sizes
drawn on the device.  tests/test_config_cases.py shows on the CPU that each case's oracle result differs from the default
configuration's, so a kernel with a default folded into a constant fails here.

The bar is the project's: bit for bit, through `done` and the auto-reset call, with the comparisons of
test_parity_gpu.py and test_settle_variants_gpu.py; every case asserts the settle variant that ran."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import config_cases as C
from test_parity_gpu import _cmp_step
from test_settle_variants_gpu import _cmp_exact

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', C.CASES, ids=C.IDS)
def test_config_case_matches_the_oracle_bit_for_bit(ref_pool, oracle_mod, monkeypatch, case):
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  if case.variant is None:
    monkeypatch.delenv('SRL_STEP_VARIANT', raising=False)
  else:
    monkeypatch.setenv('SRL_STEP_VARIANT', case.variant)
  kw = C.kw(case)
  g = envs.VecStackEnv(n_parallel=case.n, seed=C.ENV_SEED, pool=ref_pool, block=True, episode_length=case.L, **kw)
  o = oracle_mod.OracleEnv(StackConfig(n_envs=case.n, episode_length=case.L, **kw), ref_pool, seed=C.ENV_SEED)
  try:
    k = C.kernel(case)
    assert g.step_variant() == C.SHAPE[k] + (k,), '{}: variant {} ran instead of {}'.format(case.name, g.step_variant(), k)
    if 'object_max_dimension' in kw:                 # the object maps are rendered at load time with the pixel size of this config
      for m in range(len(ref_pool)):
        assert np.array_equal(g.object_map(m), o.render_object(m)), 'mesh {}'.format(m)
    drv = C.Driver(case, g.config, len(ref_pool))
    drv.start([g, o])
    gout, oout = g.reset(), o.reset()
    assert np.array_equal(gout[0][0].cpu().numpy(), oout[0][0]) and np.array_equal(gout[0][1].cpu().numpy(), oout[0][1])
    assert np.array_equal(g.maps()[2], o.maps()[2]), 'goal rectangles at reset'
    done_at = []
    for t in range(C.n_calls(case)):
      a = drv.actions([g, o])
      gout = g.step(torch.from_numpy(a).cuda())
      oout = o.step(a)
      tag = '{} call {}'.format(case.name, t)
      assert o.rc == 0, tag
      _cmp_step(g, o, gout, oout, tag)
      _cmp_exact(g, o, range(case.n), tag)
      assert np.array_equal(gout[1].cpu().numpy().view(np.uint32), oout[1].view(np.uint32)), tag + ': reward bits'
      if oout[2].all():
        done_at.append(t)
      else:
        assert not oout[2].any(), tag
    assert done_at == list(range(case.L - 1, C.n_calls(case), case.L + 1)), done_at    # every episode ran to `done`
  finally:
    g.close()
    o.close()
