"""CPU tests of the heuristic baselines' batch-wise choice over the object maps of a Stack-v2 observation
(include/stackrl_baseline_rows.h) as `baselines.baseline_rows_reference` restates it, against what the reference's own
`Baseline(batched=True, batchwise=True)` returned (tests/golden/make_baselines_v2_golden.py -> baselines_v2_golden.npz).

The value maps and masks fed to the restatement come from oracle/baselines_oracle.py.  Rows and actions are integers and must
be equal.  `height` is a maximum of exact sums, so its numbers must be equal too; the float64 sums of the other methods are
taken in another order than numpy's, so their numbers (c and the returned maps) are held to rtol 1e-12, the tolerance
tests/test_baselines.py uses for the same functions' returned maps."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'baselines_v2_golden.npz')
SHAPES = {'s32': (32, 8, 4, 6), 's64': (64, 16, 8, 2)}      # H, h, G, envs


@pytest.fixture(scope='module')
def fix():
  return np.load(FIX)


@pytest.fixture(scope='module')
def oracle_maps(fix):
  """{(tag, method): (values [B, G, OH, OH], mask [B, G, OH, OH])} from the oracle, computed once."""
  from oracle import baselines_oracle as O
  out = {}
  for tag in fix['shapes']:
    m, o = fix[tag + '/obs_map'], fix[tag + '/obs_obj']
    B, G = o.shape[:2]
    mask = np.stack([np.stack([O.goal_overlap((m[b], o[b, r])) for r in range(G)]) for b in range(B)])
    for method in fix['methods']:
      vals = np.stack([np.stack([O.METHODS[str(method)]((m[b], o[b, r])) for r in range(G)]) for b in range(B)])
      out[(str(tag), str(method))] = (vals, mask)
  return out


def _close(method, got, ref):
  return np.array_equal(got, ref) if method == 'height' else np.allclose(got, ref, rtol=1e-12, atol=0)


def test_fixture_is_what_the_issue_describes(fix):
  assert [str(t) for t in fix['shapes']] == ['s32', 's64'] and len(fix['methods']) == 4
  for tag, (H, h, G, B) in SHAPES.items():
    assert fix[tag + '/obs_map'].shape == (B, H, H, 2) and fix[tag + '/obs_obj'].shape == (B, G, h, h, 1)
    assert fix[tag + '/obs_map'].dtype == np.uint8 and fix[tag + '/obs_obj'].dtype == np.uint8
    assert (fix[tag + '/obs_map'][..., 1].reshape(B, -1).max(1) > 0).all()           # every env has a goal
    o = fix[tag + '/obs_obj']
    for b in range(B):                                                                # no two rows of an env are the same map
      assert len({o[b, r].tobytes() for r in range(G)}) == G
  assert os.path.getsize(FIX) < 300 * 1024
  for k in fix.files:
    if fix[k].dtype.kind in 'fiu':
      assert np.all(np.isfinite(fix[k])), k


def test_reference_row_differs_from_the_plain_arg_min_in_a_third_of_the_cases(fix):
  differ = total = 0
  for tag in fix['shapes']:
    for method in fix['methods']:
      for mo in fix['minorders']:
        rows = fix['{}/{}/g1_m{}/row'.format(tag, method, mo)]
        differ += int((rows != fix['{}/{}/plain_row'.format(tag, method)]).sum()); total += len(rows)
  assert total == 8 * 4 * 2 and 3 * differ >= total, (differ, total)


def test_plain_rows_of_the_fixture_are_the_oracles(fix, oracle_maps):
  for (tag, method), (vals, _) in oracle_maps.items():
    B, G = vals.shape[:2]
    plain = vals.reshape(B, -1).argmin(1) // (vals.shape[2] * vals.shape[3])
    assert np.array_equal(plain, fix['{}/{}/plain_row'.format(tag, method)]), (tag, method)


def test_restatement_matches_the_reference(fix, oracle_maps):
  from stackrl_amd.baselines import baseline_rows_reference
  g_maps, mo_maps = (int(x) for x in fix['maps_config'])
  n_maps = 0
  for (tag, method), (vals, mask) in oracle_maps.items():
    A = vals.shape[2] * vals.shape[3]
    for goal in (True, False):
      for mo in (int(x) for x in fix['minorders']):
        key = '{}/{}/g{}_m{}'.format(tag, method, int(goal), mo)
        actions, c, neg = baseline_rows_reference(vals, mask if goal else None, goal=goal, minorder=mo)
        assert np.array_equal(actions // A, fix[key + '/row']), key
        assert np.array_equal(actions % A, fix[key + '/action']), key
        assert _close(method, c, fix[key + '/c']), key
        if (int(goal), mo) == (g_maps, mo_maps):
          ref = fix[key + '/maps']
          assert _close(method, neg.reshape(ref.shape), ref), key
          n_maps += 1
  assert n_maps == 8                                               # one configuration per method and shape


def _rows(*maps):
  v = np.stack([np.asarray(m, np.float64) for m in maps])[None]
  return v, np.ones(v.shape, bool)


def tie_cases():
  """(what, values [1, G, 3, 3], expected row).  Y reaches a lower minimum than X: the better row."""
  rng = np.random.RandomState(3)
  X = 2.0 + rng.rand(3, 3)
  Y = 1.0 + rng.rand(3, 3)
  Y[1, 1] = 0.25
  Y2 = Y.T.copy()                                                  # the same best value at the same pixel, another map
  return [('X Y Y', _rows(X, Y, Y)[0], 1), ('Y Y', _rows(Y, Y)[0], 0), ('X Y Y2', _rows(X, Y, Y2)[0], 1), ('Y X', _rows(Y, X)[0], 0)]


@pytest.mark.parametrize('goal,minorder', [(True, 1), (True, 0), (False, 1)])
def test_ties_between_rows_go_to_the_first(goal, minorder):
  from stackrl_amd.baselines import baseline_rows_reference
  for what, v, row in tie_cases():
    actions, c, neg = baseline_rows_reference(v, np.ones(v.shape, bool), goal=goal, minorder=minorder)
    assert actions[0] == row * 9 + 4, (what, actions)              # the chosen row is a Y: its 0.25 at pixel (1, 1)
    assert c[0, row] == c[0].max() and (c[0, :row] < c[0, row]).all(), what


def test_n_valid_equals_the_first_rows_alone(fix, oracle_maps):
  from stackrl_amd.baselines import baseline_rows_reference
  vals, mask = oracle_maps[('s64', 'difference')]
  G = vals.shape[1]
  for k in (1, 3, G - 1, G):
    a, c, neg = baseline_rows_reference(vals, mask, n_valid=k)
    a2, c2, neg2 = baseline_rows_reference(vals[:, :k], mask[:, :k])
    assert np.array_equal(a, a2) and np.array_equal(c[:, :k], c2) and np.array_equal(neg[:, :k], neg2)
    assert np.isneginf(c[:, k:]).all() and np.isneginf(neg[:, k:]).all()
    poisoned = vals.copy(); poisoned[:, k:] = np.nan               # rows from n_valid on are not read
    assert np.array_equal(baseline_rows_reference(poisoned, mask, n_valid=k)[0], a)


def test_argument_errors():
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  v = np.random.RandomState(0).rand(2, 3, 5, 5)
  m = np.ones(v.shape, bool)
  for bad in (0, 4, -1):
    with pytest.raises(ValueError, match='n_valid'):
      Bd.baseline_rows_reference(v, m, n_valid=bad)
  with pytest.raises(ValueError):
    Bd.baseline_rows_reference(v[0], m[0])
  with pytest.raises(ValueError, match='mask'):
    Bd.baseline_rows_reference(v, None, goal=True)
  xm = torch.zeros((2, 16, 16, 2), dtype=torch.uint8)
  for shape in ((2, 4, 4), (2, 3, 1, 4, 4, 1)):                    # rank 3 and rank 6 object maps
    with pytest.raises(ValueError, match='object maps'):
      Bd.heuristic_values('height', (xm, torch.zeros(shape, dtype=torch.uint8)))
    with pytest.raises(ValueError, match='object maps'):
      Bd.Baseline('height')((xm, torch.zeros(shape, dtype=torch.uint8)))
  for bad in (0, 4):                                               # refused before a device is asked for
    with pytest.raises(ValueError, match='n_valid'):
      Bd.heuristic_values('height', (xm, torch.zeros((2, 3, 4, 4, 1), dtype=torch.uint8)), n_valid=bad)
  with pytest.raises(ValueError, match='uint8'):
    Bd.heuristic_values('height', (xm, torch.zeros((2, 3, 4, 4, 1), dtype=torch.float32)))
  with pytest.raises(ValueError):
    Bd.select(torch.zeros((2, 3)))


def test_qnet_library_exports_the_row_entry_points():
  from stackrl_amd import build
  build.build()
  with open(os.path.join(ROOT, 'include', 'stackrl_baseline_rows.h')) as f:
    names = sorted(set(re.findall(r'\b(srl_[a-z0-9_]+)\s*\(', f.read())))
  assert {'srl_baseline_rows_select', 'srl_heuristic_rows'} <= set(names)     # and those the comment points to
  L = ctypes.CDLL(build.QLIB)
  for n in names:
    assert hasattr(L, n), 'missing export ' + n
  assert any(d.endswith('stackrl_baseline_rows.h') for d in build.deps('qnet'))
