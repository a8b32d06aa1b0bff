"""CPU tests of the policy comparison (stackrl_amd/compare.py) against what the reference's `stackrl/test.py` returned on the
scripted envs and policies of tests/compare_cases.py (tests/golden/compare_golden.npz, written by
tests/golden/make_compare_golden.py): the restatement of include/stackrl_compare.h and the torch CPU path against `analyse`,
`run` on one env and on three side by side against the reference's `run`, `write` against the reference's files, and wrong
variants of the definition against the maps that tell them apart."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import compare_cases as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = len(C.KEYS)
MATRICES = ('corrcoef', 'overlap_mean', 'overlap_std')


@functools.lru_cache(maxsize=None)
def golden():
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'compare_golden.npz'))
  return {k: g[k] for k in g.files}


def _policies():
  return {k: C.batched(C.VALUE_FNS[k]) for k in C.KEYS}


@functools.lru_cache(maxsize=None)
def _run(envs):
  from stackrl_amd import compare
  env = C.VecScriptedEnv(envs)
  data = compare.run(env, _policies(), num_steps=C.NUM_STEPS, seed=C.SEED, keep_values=True)
  return data, env.calls


def _clear_of_thresholds(x32):
  """The smallest distance of a value from a threshold, exact hits of a threshold that float32 holds exactly left out, and the
  number of those hits."""
  x = x32.astype(np.float64)
  mu = x.mean(-1, keepdims=True)
  sd = x.std(-1, keepdims=True)
  smallest, hits = np.inf, 0
  for thr in (mu, mu + sd):
    gap = np.abs(x - thr)
    exact = (gap == 0) & (thr.astype(np.float32).astype(np.float64) == thr)
    hits += int(exact.sum())
    smallest = min(smallest, float(gap[~exact].min()))
  return smallest, hits


def test_no_value_of_the_fixture_lies_near_a_threshold():
  """numpy's float32 means and standard deviations (what the reference compares with) and the float64 ones of the definition
  differ by a few float32 roundings of numbers below 64: far less than 1e-3.  With every value at least 1e-3 from both
  thresholds the two give the same flags, so counts and overlaps are compared exactly below."""
  g = golden()
  for e in range(len(C.ENVS)):
    gap, hits = _clear_of_thresholds(g['run{}/values'.format(e)])
    print('env', e, 'smallest gap', gap)
    assert gap > 1e-3 and hits == 0
  # the edge maps: values ON the mean (an integer: the same threshold in both precisions), everything else clear of it
  gap, hits = _clear_of_thresholds(g['edge/values'])
  print('edge maps: smallest gap', gap, 'values on a threshold', hits)
  assert gap > 1e-3 and hits > 50


def _check_matrices(got, g, prefix):
  assert np.array_equal(got['overlap_mean'], g[prefix + 'overlap_mean'])
  assert np.array_equal(got['overlap_std'], g[prefix + 'overlap_std'])
  err = np.abs(got['corrcoef'] - g[prefix + 'corrcoef']).max()
  print(prefix, 'corrcoef: largest difference from np.corrcoef', err)
  assert err <= 1e-12


@pytest.mark.parametrize('source', ['run0', 'run1', 'run2', 'edge'])
def test_restatement_and_torch_path_against_the_reference_analysis(source):
  from stackrl_amd import compare
  g = golden()
  values = g['edge/values64'] if source == 'edge' else g[source + '/values']        # [P, T, A]
  prefix = 'edge_analyse/' if source == 'edge' else source.replace('run', 'analyse') + '/'
  record, amax = compare.compare_reference(values)
  assert record.shape == (compare.record_doubles(P),) and record[0] == values.shape[1]
  assert np.array_equal(amax, values.astype(np.float32).max(-1))
  _check_matrices(compare.matrices(record, P, C.A), g, prefix)
  # the torch path, fed step by step (B = 1) and as one step of T envs, float32 and float64 inputs mixed
  for chunks in (values.shape[1], 1):
    st = compare.MapStatistics(P, C.A)
    out = []
    for t in np.array_split(np.arange(values.shape[1]), chunks):
      out.append(st.step([torch.from_numpy(values[j][t]).to(torch.float64 if j == 1 or source == 'edge' else torch.float32) for j in range(P)]))
    assert np.array_equal(torch.cat(out, 1).numpy(), amax)
    rec = st.result()
    r, w = compare.unpack(rec, P), compare.unpack(record, P)
    for k in ('samples', 'I1', 'U1', 'I2', 'U2'):
      assert np.array_equal(r[k], w[k]), k
    if source != 'edge':                      # integer maps: every sum is exact
      assert np.array_equal(rec, record)
    _check_matrices(compare.matrices(rec, P, C.A), g, prefix)
  u = compare.unpack(record, P)
  assert np.array_equal(u['S'], u['S'].T) and np.array_equal(np.diag(u['I1']), np.diag(u['U1']))


def _against_reference_run(data, b, g, e):
  from stackrl_amd import compare
  ref = compare.to_reference(data, b)
  for k in ('keys', 'actions', 'values', 'rewards', 'episode_bounds'):
    want = g['run{}/{}'.format(e, k)]
    assert ref[k].dtype == want.dtype and np.array_equal(ref[k], want), k
  assert np.array_equal(data['action_values'][:, :, b], g['run{}/values'.format(e)].max(-1))


@pytest.mark.parametrize('e', [0, 1, 2])
def test_run_on_one_env_equals_the_reference_run_and_analysis(e):
  from stackrl_amd import compare
  g = golden()
  data, calls = _run((C.ENVS[e],))
  _against_reference_run(data, 0, g, e)
  # the reset calls are not steps: P * num_steps steps and one more call per finished episode
  assert calls == P * C.NUM_STEPS + int(data['dones'].sum())
  assert np.array_equal(data['record'], compare.compare_reference(data['values'][:, :, 0])[0])
  res = compare.analyse(data)
  assert list(res['keys']) == list(C.KEYS)
  for k in ('return', 'return_std', 'action_value', 'action_value_std'):
    want = g['analyse{}/{}'.format(e, k)]
    assert res[k].dtype == want.dtype == np.float32 and res[k].shape == want.shape
    # float32 statistics of at most 36 numbers below 64: the same numpy calls, a few roundings if the order differs
    assert np.allclose(res[k], want, rtol=4 * 2.0 ** -23, atol=4 * 2.0 ** -23), k
  assert np.array_equal(res['return'], want_returns(g, e))
  assert np.array_equal(res['distance'], g['analyse{}/distance'.format(e)])
  _check_matrices(res, g, 'analyse{}/'.format(e))


def want_returns(g, e):
  """The episodes' returns from the reference's rewards and bounds (multiples of 1/4: exact), a trailing partial episode counted."""
  rewards, bounds = g['run{}/rewards'.format(e)], g['run{}/episode_bounds'.format(e)].astype(int)
  rets = [[] for _ in range(P)]
  for s, t in zip(bounds[:-1], bounds[1:]):
    rets[s // C.NUM_STEPS].append(rewards[s // C.NUM_STEPS, s % C.NUM_STEPS:s % C.NUM_STEPS + t - s].sum())
  assert g['analyse{}/return'.format(e)].tolist() == [np.float32(np.mean(np.array(r, np.float32))) for r in rets]
  return g['analyse{}/return'.format(e)]


def test_run_on_three_envs_equals_the_three_reference_runs():
  from stackrl_amd import compare
  g = golden()
  data, calls = _run(C.ENVS)
  assert data['actions'].shape == (P, P * C.NUM_STEPS, 3, 2) and data['values'].shape == (P, P * C.NUM_STEPS, 3, C.A)
  for b in range(3):
    _against_reference_run(data, b, g, b)
  # envs with episodes of 5 and of 4 steps side by side: a reset call whenever any env finished
  assert calls == P * C.NUM_STEPS + int(data['dones'].any(-1).sum())
  record, _ = compare.compare_reference(data['values'].reshape(P, -1, C.A))
  assert np.array_equal(data['record'], record)
  res = compare.analyse(data)
  rets = np.stack([g['analyse{}/return'.format(e)] for e in range(3)])       # three episodes per policy in every env
  assert np.allclose(res['return'], rets.mean(0), rtol=1e-6)
  assert np.array_equal(res['distance'], np.mean([g['analyse{}/distance'.format(e)] for e in range(3)], axis=0))


def test_write_against_the_reference_files(tmp_path):
  from stackrl_amd import compare
  g = golden()
  for tag, name, kwargs, force in C.write_calls():
    path = str(tmp_path / 'csv' / (name + '.csv'))
    want = str(g['write/{}/error'.format(tag)])
    if want:
      with pytest.raises(ValueError) as err:
        compare.write(path, force=force, **kwargs)
      assert str(err.value) == want
    else:
      compare.write(path, force=force, **kwargs)
    with open(path) as f:
      assert f.read() == str(g['write/{}/text'.format(tag)]), tag


# ------------------------------------------------------------------------------------------------ wrong variants
def _variant(values, ddof=0, strict=True, union_sum=False, rounded=True):
  """The overlaps of `analyse` with switches for the mistakes a restatement can make."""
  x = np.asarray(values, np.float64)
  if rounded:
    x = x.astype(np.float32).astype(np.float64)
  mu = x.mean(-1, keepdims=True)
  sd = x.std(-1, ddof=ddof, keepdims=True)
  out = []
  for thr in (mu, mu + sd):
    f = (x > thr if strict else x >= thr).reshape(x.shape[0], -1)
    inter = np.array([[np.count_nonzero(a & b) for b in f] for a in f], np.float64)
    n = f.sum(-1).astype(np.float64)
    union = n[:, None] + n[None] if union_sum else np.array([[np.count_nonzero(a | b) for b in f] for a in f], np.float64)
    out.append(inter / union)
  return out


def test_wrong_variants_differ_from_the_reference():
  g = golden()
  v = g['edge/values64']
  want = [g['edge_analyse/overlap_mean'], g['edge_analyse/overlap_std']]
  right = _variant(v)
  assert np.array_equal(right[0], want[0]) and np.array_equal(right[1], want[1])
  assert not np.array_equal(_variant(v, ddof=1)[1], want[1])
  assert not np.array_equal(_variant(v, strict=False)[0], want[0])
  assert not np.array_equal(_variant(v, union_sum=True)[0], want[0]) and not np.array_equal(_variant(v, union_sum=True)[1], want[1])
  assert not np.array_equal(_variant(v, rounded=False)[0], want[0])
  for e in range(len(C.ENVS)):                # the union as a sum shows on the scripted runs as well
    assert not np.array_equal(_variant(g['run{}/values'.format(e)], union_sum=True)[0], g['analyse{}/overlap_mean'.format(e)])


def test_arguments_are_checked():
  from stackrl_amd import compare
  with pytest.raises(ValueError):
    compare.MapStatistics(0, 81)
  with pytest.raises(ValueError):
    compare.MapStatistics(9, 81)
  with pytest.raises(ValueError):
    compare.MapStatistics(2, 0)
  st = compare.MapStatistics(2, 4)
  with pytest.raises(ValueError):
    st.step([torch.zeros(3, 4)])
  with pytest.raises(ValueError, match='rows'):
    st.step([torch.zeros(3, 8), torch.zeros(3, 8)])
  with pytest.raises(TypeError):
    compare.run(C.VecScriptedEnv(C.ENVS[:1]), {'a': 1})
  # grouped maps: the chosen row's map
  a = [torch.tensor([5, 0, 7]), torch.tensor([0, 4, 3])]
  maps = [torch.arange(24.).reshape(3, 8), -torch.arange(24.).reshape(3, 8).double()]
  amax = st.step(maps, a)
  rows = [torch.stack([m.reshape(3, 2, 4)[b, int(a[j][b]) // 4] for b in range(3)]) for j, m in enumerate(maps)]
  assert torch.equal(amax, torch.stack([r.float().amax(-1) for r in rows]))
  assert np.array_equal(st.result(), compare.compare_reference(rows)[0])
