"""Env configurations away from the defaults, shared by tests/test_config_cases.py (CPU: the oracle alone — every case
changes what the oracle computes, so a kernel that ignored the field could not pass) and tests/test_config_parity_gpu.py
(the HIP path against the oracle, bit for bit).

`srl_config` (include/srl_types.h) is read at run time by the settle, reward and goal code; the other parity tests build
their envs with its defaults.  A case is plain data:

  name      test id
  fixed     StackConfig kwargs that the case and the run it must differ from share (the rewarder, Stack-v2 freedoms, ...)
  varied    the StackConfig kwargs under test; left out, StackConfig's defaults take their place (`base_kw`)
  L, n      episode length, env count
  variant   settle launch variant to force through SRL_STEP_VARIANT: None, 'four_wave', 'two_wave'
  drive     'pile': settle_scenarios.pile_script / pile_actions with scripted goals, L + 2 calls (through `done` and the
            auto-reset call); 'rng': no script, `sample()`, goals from the env's RNG, two whole episodes (2 (L + 1) calls:
            the second episode's meshes and goal are drawn by the auto-reset)
  differs   what must differ from the `base_kw` run on the oracle: 'poses', 'reward' or 'goal'

Every committed case keeps status 0 in every env on the oracle (no divergence: solver_iterations = 1 and friction_rock = 0
are left out for that reason).  numpy only."""
import collections

import numpy as np

import settle_scenarios as S

Case = collections.namedtuple('Case', 'name fixed varied L n variant drive differs')

# stackrl_amd.config.SOLVER_PRESETS['bullet10'], restated so that a change to the preset shows in test_config_cases.py
BULLET10 = dict(solver_iterations=10, warmstart=0.85, linear_slop=0.0, residual_threshold=0.0)
# one of everything the placement and the sub-step read besides the solver's own four
MIXED = dict(place_at_com=False, friction_rock=0.9, friction_ground=0.2, linear_damping=0.2, angular_damping=0.0, gravity=19.6,
             velocity_threshold=0.03, erp=0.35, collision_margin=0.002)

# the sweep cap of a case whose sub-steps must nearly all leave the sweep loop at the cap (name -> solver_iterations)
CAP_CASES = {'bullet10': 10, 'solver_iterations-4': 4, 'residual_threshold-0': 50}

K_STEP, K_PP1, K_PP2, K_T128 = 0, 1, 2, 3      # srl_get_step_variant's kernel ids
SHAPE = {K_STEP: (128, 1), K_PP1: (256, 1), K_PP2: (256, 2), K_T128: (128, 2)}   # (threads, points per thread)


def _solver(name, **varied):
  return Case(name, {}, varied, 6, 4, None, 'pile', 'poses')


SOLVER = [
  _solver('bullet10', **BULLET10),
  _solver('solver_iterations-4', solver_iterations=4),
  _solver('residual_threshold-0', residual_threshold=0.0),
  _solver('warmstart-0', warmstart=0.0),
  _solver('warmstart-1', warmstart=1.0),
  _solver('linear_slop-0', linear_slop=0.0),
  _solver('erp-0.35', erp=0.35),
  _solver('collision_margin-0.002', collision_margin=0.002),
  _solver('friction-0.9-0.2', friction_rock=0.9, friction_ground=0.2),
  _solver('damping-0.2-0', linear_damping=0.2, angular_damping=0.0),
  _solver('gravity-19.6', gravity=19.6),
  _solver('velocity_threshold-0.03', velocity_threshold=0.03),
  _solver('sim_time_step-0.02', sim_time_step=0.02),
  _solver('object_max_dimension-0.15', object_max_dimension=0.15),
  _solver('place_at_com-False', place_at_com=False),
]

VARIANTS = [Case('{}-L{}{}'.format(nm, L, '-' + v if v else ''), {}, kw, L, n, v, 'pile', 'poses')
            for nm, kw in (('bullet10', BULLET10), ('solver_iterations-4', dict(solver_iterations=4)), ('mixed', MIXED))
            for L, n, v in ((12, 3, 'four_wave'), (12, 3, 'two_wave'), (17, 2, None))]

STACK_V2 = [
  Case('v2-orient2-place_at_com-False', dict(orientation_freedom=2), dict(place_at_com=False), 5, 4, None, 'rng', 'poses'),
  Case('v2-orient1-ordering-place_at_com-False', dict(orientation_freedom=1, ordering_freedom=True), dict(place_at_com=False),
       5, 4, None, 'rng', 'poses'),
]

REWARD = [Case('reward_params-{}'.format(nm), dict(rewarder='all'), dict(reward_params=p), 6, 6, None, 'pile', 'reward')
          for nm, p in (('None', None), ('1-3', (1, 3)), ('0-2', (0, 2)), ('3', 3))]
REWARD.append(Case('reward_params-1-3-dor-scalar', dict(rewarder='dor', reward_scale=None), dict(reward_params=(1, 3)), 6, 6, None,
                   'pile', 'reward'))

GOAL = [Case('goal_size_ratio-{}'.format(r), dict(rewarder='all'), dict(goal_size_ratio=r), 4, 16, None, 'rng', 'goal')
        for r in (0.1, 0.5, 0.9, 1.0, 0.0625)]
GOAL.append(Case('goal_size_ratio-0.1-rf4', dict(rewarder='all', resolution_factor=4), dict(goal_size_ratio=0.1), 4, 16, None, 'rng',
                 'goal'))

CASES = SOLVER + VARIANTS + STACK_V2 + REWARD + GOAL
IDS = [c.name for c in CASES]
ENV_SEED = S.ENV_SEED


def kw(case):
  """StackConfig / VecStackEnv kwargs of the case (without n_envs / n_parallel and episode_length)."""
  return dict(case.fixed, **case.varied)


def base_kw(case):
  """The run the case must differ from: the varied fields at StackConfig's defaults."""
  return dict(case.fixed)


def kernel(case):
  """The settle kernel the case must run (`step_variant()[2]`): by episode length unless a variant is forced."""
  if case.variant is not None:
    assert 9 <= case.L <= 16, 'SRL_STEP_VARIANT chooses between the two kernels of 9 - 16 rocks'
    return {'four_wave': K_PP1, 'two_wave': K_T128}[case.variant]
  return K_STEP if case.L <= 8 else K_PP1 if case.L <= 16 else K_PP2


def n_calls(case):
  return case.L + 2 if case.drive == 'pile' else 2 * (case.L + 1)


class Driver(object):
  """The actions of a case, call by call, for any number of envs run side by side (the HIP env and the oracle, or the
  oracle under two configurations).  `start(envs)` scripts them (pile drive) — call it before their reset; `actions(envs)`
  returns one call's actions as int64 [n]: the pile script's, or `sample()` of every env, which must agree."""

  def __init__(self, case, cfg, pool_size):
    self.case = case
    self.aw = cfg.overhead_res - cfg.object_res + 1
    if case.drive == 'pile':
      self.ids, self.rect, self.rng = S.pile_script(pool_size, case.n, case.L)
    else:
      assert case.drive == 'rng', case.drive

  def start(self, envs):
    if self.case.drive == 'pile':
      for e in envs:
        e.set_script(self.ids, self.rect)

  def actions(self, envs):
    if self.case.drive == 'pile':
      return S.pile_actions(self.rng, self.case.n, self.aw)
    a = [e.sample() for e in envs]
    a = [np.asarray(x.cpu() if hasattr(x, 'cpu') else x, np.int64) for x in a]     # (the HIP env returns a device tensor)
    for b in a[1:]:
      assert np.array_equal(a[0], b), 'sample() differs between the envs of one case'
    return a[0]
