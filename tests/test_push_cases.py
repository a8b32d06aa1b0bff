"""CPU tests of the push test's definition (include/stackrl_hip.h "Push test") as tests/push_cases.py restates it: the restated
perr / oerr against the oracle's `srlo_distance_from_place` bit for bit on random and on closed-form pose pairs, hand-made
piles that tell six wrong readings of the definition apart, and one physical check on the oracle alone — a kicked rock slides
the Coulomb distance."""
import ctypes

import numpy as np
import pytest

import push_cases as pc
from stackrl_amd.config import StackConfig

F32 = np.float32


def _p(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _oracle_distance(L, ref7, now7):
  ref7, now7, out = np.ascontiguousarray(ref7, F32), np.ascontiguousarray(now7, F32), np.zeros(2, F32)
  L.srlo_distance_from_place(_p(ref7), _p(now7), _p(out))
  return out


def _bits(a):
  return np.ascontiguousarray(a, F32).view(np.int32)


def _unit(q):
  return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(F32)


def test_restated_distance_equals_the_oracle_on_random_pose_pairs(oracle_mod):
  L = oracle_mod.lib()
  rng = np.random.RandomState(7)
  n = 2400
  ref = np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)), _unit(rng.normal(size=(n, 4)))], 1).astype(F32)
  now = np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)), _unit(rng.normal(size=(n, 4)))], 1).astype(F32)
  # a third close to their reference (what a settled pile looks like: dw at and around 1), some beyond it after rounding
  near = slice(0, n // 3)
  now[near, :3] = ref[near, :3] + rng.normal(scale=1e-4, size=(n // 3, 3)).astype(F32)
  now[near, 3:] = _unit(ref[near, 3:] + rng.normal(scale=1e-4, size=(n // 3, 4)).astype(F32))
  now[:40, 3:] = ref[:40, 3:] * F32(1.0000005)
  acos_seen = set()
  for i in range(n):
    got = pc.distance(ref[i], now[i])
    want = _oracle_distance(L, ref[i], now[i])
    assert np.array_equal(_bits(got), _bits(want)), (i, got, want)
    acos_seen.add(float(got[1]) > 1.0)
  assert acos_seen == {False, True}
  for x in np.concatenate([rng.uniform(-1.2, 1.2, 500), [0.0, 1.0, -1.0, 0.5]]).astype(F32):
    assert _bits(pc.acos(x)) == _bits(F32(L.srlo_acosf(ctypes.c_float(x)))), x


def test_restated_distance_on_closed_form_pairs(oracle_mod):
  L = oracle_mod.lib()
  q = _unit(np.array([0.1, -0.3, 0.2, 0.9]))
  pose = np.concatenate([F32([0.2, 0.3, 0.05]), q])
  # quaternions whose squared norm is 1 exactly in float32: there "the same orientation" is 0 exactly
  x = F32([0.2, 0.3, 0.05])
  unit = [np.concatenate([x, F32(u)]) for u in ([0, 0, 0, 1], [0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, -0.5])]
  half_turn = L.srlo_acosf(ctypes.c_float(0.0))
  cases = [(u, u, F32(0), F32(0)) for u in unit]                                    # identical
  cases += [(u, np.concatenate([x, -u[3:]]), F32(0), F32(0)) for u in unit]         # q and -q are one orientation
  cases += [
    (pose, pose, F32(0), None),
    (unit[0], np.concatenate([x, F32([0, 0, 1, 0])]), F32(0), F32(2) * F32(half_turn)),   # a half turn about z
    (unit[1], np.concatenate([x, F32([0.5, 0.5, -0.5, -0.5])]), F32(0), F32(2) * F32(half_turn)),
    (pose, np.concatenate([pose[:3] + F32([0.03, 0.04, 0.0]), q]), None, None),     # a 3-4-5 translation
  ]
  for k, (a, b, perr, oerr) in enumerate(cases):
    got = pc.distance(a, b)
    assert np.array_equal(_bits(got), _bits(_oracle_distance(L, a, b))), k
    if perr is not None:
      assert got[0] == perr, k
    if oerr is not None:
      assert got[1] == F32(oerr), k
  # |q|^2 of a float32 quaternion is 1 only to rounding (4 products and sums: within 4 x 2^-24), and acos(1 - e) is about
  # sqrt(2 e): identical and opposite orientations give the same small angle
  assert pc.distance(pose, pose)[1] == pc.distance(pose, np.concatenate([pose[:3], -q]))[1] <= 2 * np.sqrt(2 * 4 * 2.0 ** -24) * 1.6
  d = pc.distance(cases[-1][0], cases[-1][1])[0]
  assert abs(float(d) - 0.05) <= 4 * 2.0 ** -24 and d == pc.distance(cases[-1][1], cases[-1][0])[0]
  assert F32(2) * F32(half_turn) == pytest.approx(np.pi, abs=2e-4)                  # (the polynomial's own error, A&S: 2e-8 x 2 ... float32)


# ------------------------------------------------------------------------------------------------ hand-made piles
L_ = 5


def _pile(nb):
  """A pile of L_ slots: distinct poses, place poses, velocities; slots at or above nb hold stale words, as a blob may."""
  rng = np.random.RandomState(3)
  poses = np.zeros((L_, 8), F32)
  poses[:, :3] = rng.uniform(0.1, 0.4, (L_, 3))
  poses[:, 3:7] = _unit(rng.normal(size=(L_, 4)))
  poses[:, 7] = np.arange(L_)
  place = poses[:, :7].copy()
  place[:, :3] += rng.normal(scale=[1e-3, 3e-3, 1e-2, 3e-2, 1e-1], size=(3, L_)).T.astype(F32)
  place[:, 3:7] = _unit(place[:, 3:7] + rng.normal(scale=0.05, size=(L_, 4)))
  vel = np.zeros((L_, 8), F32)
  vel[:, 0:3] = rng.normal(scale=0.1, size=(L_, 3))
  vel[:, 4:7] = rng.normal(scale=1.0, size=(L_, 3))
  return poses, vel, place, nb


def _differs(x, y):
  return any(not pc.same_bits(a, b) for a, b in zip(x, y))


def test_cases_tell_wrong_readings_apart():
  poses, vel, place, nb = _pile(3)
  tol = (2e-3, 0.05)
  right = pc.rows_summary(poses, vel, nb, place, tol=tol)
  assert right[1][0] == 3 and 0 < right[1][1] <= 3 and not right[0][nb:].any()
  # no fabsf: a pile whose quaternions sit in the other hemisphere than their place quaternions
  flipped = poses.copy()
  flipped[:, 3:7] = -flipped[:, 3:7]
  assert pc.same_bits(pc.rows_summary(flipped, vel, nb, place, tol=tol)[0], right[0])
  assert _differs(pc.rows_summary(flipped, vel, nb, place, tol=tol, variant='no_fabs'), right)
  # slots <= nb instead of < nb
  assert _differs(pc.rows_summary(poses, vel, nb, place, tol=tol, variant='slots_le_nb'), right)
  # the sum in another order: magnitudes 1e-3 .. 1e-1 do not add up alike both ways
  poses5, vel5, place5, _ = _pile(5)
  fwd, rev = pc.rows_summary(poses5, vel5, 5, place5, tol=tol), pc.rows_summary(poses5, vel5, 5, place5, tol=tol, variant='sum_reversed')
  assert pc.same_bits(fwd[0], rev[0]) and fwd[1][4] != rev[1][4] and pc.same_bits(np.delete(fwd[1], 4), np.delete(rev[1], 4))
  # a NaN counts as moved, and the maxima pass over it
  nan = poses.copy()
  nan[1, 0] = np.nan
  with_nan = pc.rows_summary(nan, vel, nb, place, tol=(10.0, 10.0))
  assert np.isnan(with_nan[0][1, 0]) and with_nan[1][1] == 1 and np.isnan(with_nan[1][4]) and with_nan[1][2] == max(right[0][0, 0], right[0][2, 0])
  assert pc.rows_summary(nan, vel, nb, place, tol=(10.0, 10.0), variant='nan_not_moved')[1][1] == 0
  # ref_nb: a body the reference does not hold yet is measured from its place pose
  ref = poses.copy()
  ref[:, :3] += F32(0.01)
  held = pc.rows_summary(poses, vel, nb, place, ref=ref, ref_nb=2, tol=tol)
  assert pc.same_bits(held[0][2], right[0][2]) and not pc.same_bits(held[0][:2], right[0][:2])
  assert _differs(pc.rows_summary(poses, vel, nb, place, ref=ref, ref_nb=2, tol=tol, variant='ref_nb_ignored'), held)
  assert pc.same_bits(pc.rows_summary(poses, vel, nb, place, ref=ref, ref_nb=None, tol=tol)[0],
                      pc.rows_summary(poses, vel, nb, place, ref=ref, ref_nb=3, tol=tol)[0])
  # dz, speed, spin, min dz in plain terms
  assert right[0][0, 2] == F32(poses[0, 2] - place[0, 2]) and right[1][5] == min(0.0, right[0][:nb, 2].min())
  assert right[0][0, 3] == pytest.approx(np.linalg.norm(vel[0, :3]), rel=1e-6)
  assert right[1][7] == pytest.approx(np.linalg.norm(vel[:nb, 4:7], axis=1).max(), rel=1e-6)


def test_kick_selection_and_layouts():
  _, vel, _, nb = _pile(3)
  rng = np.random.RandomState(5)
  dv = rng.normal(size=(L_, 8)).astype(F32)
  per = pc.kick(vel, nb, dv, 1, pc.KICK_ALL)
  cols = [0, 1, 2, 4, 5, 6]
  assert np.array_equal(per[:nb][:, cols], (vel[:nb][:, cols] + dv[:nb][:, cols]).astype(F32))
  assert np.array_equal(per[nb:], vel[nb:]) and np.array_equal(per[:, [3, 7]], vel[:, [3, 7]])          # untouched slots and columns
  one = pc.kick(vel, nb, dv[0], 0, pc.KICK_ALL)
  assert np.array_equal(one[:nb][:, cols], (vel[:nb][:, cols] + dv[0][cols]).astype(F32)) and np.array_equal(one[nb:], vel[nb:])
  last = pc.kick(vel, nb, dv, 1, pc.KICK_LAST)
  assert np.array_equal(np.nonzero((last != vel).any(1))[0], [nb - 1])
  assert np.array_equal(pc.kick(vel, nb, dv, 1, 1), pc.kick(pc.kick(vel, nb, dv, 1, 1), 0, dv, 1, pc.KICK_ALL))   # nb = 0: nothing
  assert np.array_equal(np.nonzero((pc.kick(vel, nb, dv, 1, 1) != vel).any(1))[0], [1])
  assert np.array_equal(pc.kick(vel, nb, dv, 1, nb), vel) and np.array_equal(pc.kick(vel, nb, dv, 1, L_ - 1), vel)   # a slot at or above nb
  assert np.array_equal(pc.kick(vel, 0, dv, 1, pc.KICK_LAST), vel) and np.array_equal(pc.kick(vel, L_ + 3, dv, 1, pc.KICK_ALL), pc.kick(vel, L_, dv, 1, pc.KICK_ALL))
  # the wrong readings
  assert not np.array_equal(pc.kick(vel, nb, dv, 1, pc.KICK_LAST, variant='last_hits_nb'), last)
  assert not np.array_equal(pc.kick(vel, nb, dv, 1, pc.KICK_ALL, variant='slots_le_nb'), per)
  assert sorted(pc.VARIANTS) == sorted(['no_fabs', 'slots_le_nb', 'last_hits_nb', 'sum_reversed', 'nan_not_moved', 'ref_nb_ignored'])


# ------------------------------------------------------------------------------------------------ physics, on the oracle alone
def test_a_kicked_rock_slides_the_coulomb_distance(oracle_mod, ref_pool):
  """A flat cuboid at rest on the ground, kicked horizontally with speed s through the oracle's velocity hook and stepped
  until `at_rest`, has slid s^2 / (2 mu g), mu = friction_rock x friction_ground: to the 5 % that
  tests/test_physics_closed_form.py gives its own sliding case against the continuum (the sub-step's discretisation)."""
  cfg = StackConfig(n_envs=1, episode_length=3)
  sim = oracle_mod.OracleEnv(cfg, ref_pool, seed=1)
  sim.set_script(np.array([[64, 65, 66]], np.int32), np.array([[40, 40, 64, 64]], np.int32))
  sim.reset()
  sim.step(np.array([48 * 97 + 48], np.int64))
  sim.step_simulation(300)
  L = cfg.episode_length
  before, nb, _, _ = sim.state()
  vel = sim.velocities()
  assert nb[0] == 1 and pc.rows_summary(before[0, :L], vel[0, :L], 1, before[0, :L, :7])[1][6] <= cfg.velocity_threshold
  s = 1.0
  dv = np.zeros(8, F32)
  dv[0] = s
  vel[0, :L] = pc.kick(vel[0, :L], nb[0], dv, 0, pc.KICK_ALL)
  sim.set_body_state(None, vel)
  for n in range(1, 201):
    sim.step_simulation(1)
    rows, summary = pc.rows_summary(sim.state()[0][0, :L], sim.velocities()[0, :L], 1, before[0, :L, :7], ref=before[0, :L], ref_nb=1,
                                    tol=(1e-3, 1e-2))
    if summary[6] <= cfg.velocity_threshold:
      break
  c = cfg.to_c()
  want = s * s / (2.0 * float(c.friction_rock) * float(c.friction_ground) * float(c.gravity))
  print('slid {:.5f} m in {} sub-steps, s^2 / (2 mu g) = {:.5f}'.format(float(rows[0, 0]), n, want))
  assert n < 200 and summary[1] == 1 and summary[0] == 1
  assert abs(float(rows[0, 0]) - want) <= 0.05 * want
  assert abs(float(rows[0, 2])) < 1e-4 and float(rows[0, 1]) < 1e-2      # it slid: neither lifted nor turned
  sim.close()


# ------------------------------------------------------------------------------------------------ the Python side, without a device
def test_push_spec_draws_horizontal_increments_of_the_given_speed():
  torch = pytest.importorskip('torch')
  from stackrl_amd.push import PushSpec, default_tol, increments, select_code
  B, k, L = 3, 4, 5
  for mode, shape in (('bump', (B, k, 8)), ('last', (B, k, 8)), ('shake', (B, k, L, 8))):
    spec = PushSpec(speed=0.25, substeps=7, mode=mode, seed=9)
    dv = spec.draw(B, k, L, 'cpu')
    assert tuple(dv.shape) == shape and dv.dtype == torch.float32
    assert torch.allclose(dv[..., 0:2].norm(dim=-1), torch.full(shape[:-1], 0.25), rtol=1e-6) and not bool(dv[..., 2:].any())
    assert torch.equal(dv, spec.draw(B, k, L, 'cpu')) and not torch.equal(dv, PushSpec(0.25, 7, mode, seed=10).draw(B, k, L, 'cpu'))
    assert spec.select == ('last' if mode == 'last' else 'all')
    assert len(torch.unique(dv[..., 0])) == dv[..., 0].numel()          # a direction of its own per env and trial (and body)
  with pytest.raises(ValueError, match='mode must be'):
    PushSpec(mode='tilt')
  assert (select_code('all'), select_code('last'), select_code(3)) == (pc.KICK_ALL, pc.KICK_LAST, 3)
  wide, per_body = increments(torch.ones(B, L, 3), B, L, torch.device('cpu'))
  assert per_body == 1 and tuple(wide.shape) == (B, L, 8) and bool((wide[..., :3] == 1).all()) and not bool(wide[..., 3:].any())
  assert increments(torch.ones(B, 8), B, L, torch.device('cpu'))[1] == 0
  tp, to = default_tol(StackConfig(n_envs=1))
  assert tp == pytest.approx(0.125 / 32) and to == pytest.approx(2 / 32)


def test_policy_score_follows_the_penalty_and_the_tie_rule():
  """A hand-given `PoseDistances` behind a stand-in lookahead: score = reward - penalty * moved / nb, ties to the lower rank."""
  torch = pytest.importorskip('torch')
  from stackrl_amd.lookahead import LookaheadPolicy
  from stackrl_amd.push import PoseDistances, PushSpec
  reward = torch.tensor([[1.0, 0.875, 0.5], [0.25, 0.25, 0.25], [0.5, 0.75, 0.625], [0.75, 0.5, 0.25]])
  moved = torch.tensor([[2.0, 0, 0], [0, 0, 0], [0, 2, 0], [2, 0, 0]])
  summary = torch.zeros(4, 3, 8)
  summary[..., 0], summary[..., 1] = 4.0, moved
  dist = PoseDistances(torch.zeros(4, 3, 4, 4), summary, 0.01)
  values = torch.arange(40, dtype=torch.float32).reshape(4, 10)
  asked = []

  class Stub(object):
    k = 3

    def evaluate(self, cand, push=None):
      asked.append(push)
      return (reward, torch.zeros(4, 3, dtype=torch.bool)) + (() if push is None else (dist,))

  base = lambda obs: (torch.tensor([0, 1, 2, 3]), values)
  spec = PushSpec()
  plain = LookaheadPolicy(base, Stub())
  a, _ = plain(None)
  cand = plain.last[0]
  assert asked == [None] and torch.equal(a, cand[torch.arange(4), torch.tensor([0, 0, 1, 0])])
  for penalty, want in ((0.0, [0, 0, 1, 0]),
                        (0.5, [1, 0, 2, 0])):   # env 0: 0.75 < 0.875; env 2: 0.5 = 0.5 < 0.625; env 3: 0.5 ties with 0.5, lower rank
    p = LookaheadPolicy(base, Stub(), push=spec, penalty=penalty)
    a, v = p(None)
    assert asked[-1] is spec and p.last_push is dist and torch.equal(v, values)
    assert torch.equal(a, cand[torch.arange(4), torch.tensor(want)]), penalty
