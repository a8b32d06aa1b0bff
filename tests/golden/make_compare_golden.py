#!/usr/bin/env python3
"""Golden vectors for the policy comparison from the reference's own `stackrl/test.py`.

Runs only in the build container.  test.py is numpy code, but its module header imports gym, pybullet, matplotlib, `stackrl`,
`stackrl.envs` and `stackrl.heatmap`.  The functions exercised here (`run`, `analyse`, `write`) use of those only
`gym.spaces.Tuple` (an isinstance check), `plt` (drawing) and `heatmap.heatmap` (drawing a matrix), so the module is loaded by
file path with placeholders: a `gym` with an empty `spaces.Tuple` class, empty `pybullet`, `stackrl` and `stackrl.envs`, an
inert `matplotlib.pyplot` whose every function does nothing, and a `heatmap` that records the matrix it is handed.  The envs
and policies are the scripted ones of tests/compare_cases.py.  The file written (`compare_golden.npz`) holds arrays and short
strings only:
  (a) what `run` returns on each of the three one-env scripted envs;
  (b) what `analyse(save=True)` returns on those data and the four matrices it hands to `heatmap`;
  (c) the text of the files `write` leaves after each call of `compare_cases.write_calls()`;
  (d) `analyse` on hand-made maps that tell wrong definitions apart (`edge_maps`): half of them small integers whose mean is
      exactly 4, so that many values sit ON the threshold (`>` against `>=`), the others multiples of 1/64 (ddof 0 against 1),
      and a few elements of float64 maps 2^-30 above the mean, which the float32 array of the reference rounds onto it.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import compare_cases as C  # noqa: E402

REF = '/root/reference/stackrl/test.py'
OUT = os.path.join(HERE, 'compare_golden.npz')
CAPTURED = []
LABELS = {'Mean distance (pixels)': 'distance', 'Correlation coefficients': 'corrcoef', 'Overlap of values above mean': 'overlap_mean',
          'Overlap of values one std dev above mean': 'overlap_std'}


class _Inert(types.ModuleType):
  def __getattr__(self, name):
    if name.startswith('__'):
      raise AttributeError(name)
    return lambda *a, **k: None


def load_reference():
  sys.dont_write_bytecode = True   # the reference tree is read-only: no __pycache__ beside its files
  gym = types.ModuleType('gym')
  gym.spaces = types.ModuleType('gym.spaces')
  gym.spaces.Tuple = type('Tuple', (), {})
  stackrl = types.ModuleType('stackrl')
  stackrl.envs = types.ModuleType('stackrl.envs')
  stackrl.heatmap = types.ModuleType('stackrl.heatmap')

  def heatmap(data, row_labels, col_labels, cbarlabel='', **kw):
    CAPTURED.append((cbarlabel, np.array(data, copy=True)))
    return None, None
  stackrl.heatmap.heatmap = heatmap
  stackrl.heatmap.annotate_heatmap = lambda *a, **k: None
  mpl = types.ModuleType('matplotlib')
  mpl.pyplot = _Inert('matplotlib.pyplot')
  mods = {'gym': gym, 'gym.spaces': gym.spaces, 'pybullet': types.ModuleType('pybullet'), 'stackrl': stackrl,
          'stackrl.envs': stackrl.envs, 'stackrl.heatmap': stackrl.heatmap, 'matplotlib': mpl, 'matplotlib.pyplot': mpl.pyplot}
  saved = {k: sys.modules.get(k) for k in mods}
  sys.modules.update(mods)
  try:
    spec = importlib.util.spec_from_file_location('ref_test', REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
  finally:
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v
  return mod


def edge_maps(seed, P=3, T=12):
  """float64 [P, T, A]: the maps of (d)."""
  rs = np.random.RandomState(seed)
  v = np.zeros((P, T, C.A))
  for j in range(P):
    for t in range(T):
      if (j + t) % 2 == 0:
        m = rs.randint(0, 9, C.A)
        while m.sum() != 4 * C.A:                      # mean exactly 4
          i = rs.randint(C.A)
          m[i] = min(8, m[i] + 1) if m.sum() < 4 * C.A else max(0, m[i] - 1)
        v[j, t] = m
        if j == 0:
          v[j, t, np.nonzero(m == 4)[0][:2]] += 2.0 ** -30
      else:
        v[j, t] = rs.randint(0, 513, C.A) / 64.0
  return v


def gaps_ok(v32):
  """No value within 1e-3 of a threshold, unless it sits on it exactly and the threshold is the same number in float32."""
  x = v32.astype(np.float64)
  mu = x.mean(-1, keepdims=True)
  sd = x.std(-1, keepdims=True)
  for thr in (mu, mu + sd):
    gap = np.abs(x - thr)
    exact = (gap == 0) & (thr.astype(np.float32).astype(np.float64) == thr)
    if np.any((gap < 1e-3) & ~exact):
      return False
  return True


def overlaps(x, ddof=0):
  mu = x.mean(-1, keepdims=True)
  f = (x > mu + x.std(-1, ddof=ddof, keepdims=True)).reshape(x.shape[0], -1)
  return np.array([[np.count_nonzero(a & b) / np.count_nonzero(a | b) for b in f] for a in f])


def main():
  ref = load_reference()
  out = {'envs': np.array(C.ENVS), 'num_steps': np.int64(C.NUM_STEPS), 'seed': np.int64(C.SEED)}
  policies = {k: C.single(C.VALUE_FNS[k]) for k in C.KEYS}
  with tempfile.TemporaryDirectory() as tmp:
    for e, (env_id, length) in enumerate(C.ENVS):
      data = ref.run(C.ScriptedEnv(env_id, length), policies, num_steps=C.NUM_STEPS, verbose=False, seed=C.SEED)
      assert data['values'].dtype == np.float32 and np.array_equal(data['values'], np.round(data['values']))
      for k, v in data.items():
        out['run{}/{}'.format(e, k)] = v
      del CAPTURED[:]
      res = ref.analyse(**data, show=False, save=True, dirname=os.path.join(tmp, 'plots{}'.format(e)))
      for k, v in res.items():
        out['analyse{}/{}'.format(e, k)] = np.asarray(v)
      assert [LABELS[l] for l, _ in CAPTURED] == ['distance', 'corrcoef', 'overlap_mean', 'overlap_std']
      for label, m in CAPTURED:
        assert m.shape == (len(C.KEYS),) * 2 and np.all(np.isfinite(m))
        out['analyse{}/{}'.format(e, LABELS[label])] = m
    # (d): the first seed whose maps keep clear of the thresholds and on which ddof 1 moves a flag
    for dseed in range(200):
      v64 = edge_maps(dseed)
      x = v64.astype(np.float32).astype(np.float64)
      if gaps_ok(v64.astype(np.float32)) and not np.array_equal(overlaps(x), overlaps(x, ddof=1)):
        break
    else:
      raise RuntimeError('no seed found')
    P, T = v64.shape[:2]
    rs = np.random.RandomState(dseed + 1000)
    d = {'keys': np.array(C.KEYS), 'actions': rs.randint(0, 9, (P, T, 2)).astype(np.uint8), 'values': v64.astype(np.float32),
         'rewards': (rs.randint(-8, 9, (P, T // P)) / 4.0).astype(np.float32), 'episode_bounds': np.arange(0, T + 1, 2).astype(np.uint16)}
    out['edge/seed'] = np.int64(dseed)
    out['edge/values64'] = v64
    for k, v in d.items():
      out['edge/' + k] = v
    del CAPTURED[:]
    res = ref.analyse(**d, show=False, save=True, dirname=os.path.join(tmp, 'plots_edge'))
    for k, v in res.items():
      out['edge_analyse/' + k] = np.asarray(v)
    for label, m in CAPTURED:
      assert np.all(np.isfinite(m))
      out['edge_analyse/' + LABELS[label]] = m
    files = {}
    for tag, name, kwargs, force in C.write_calls():
      path = os.path.join(tmp, 'csv', name + '.csv')
      try:
        ref.write(path, force=force, **kwargs)
        out['write/{}/error'.format(tag)] = np.array('')
      except ValueError as err:
        out['write/{}/error'.format(tag)] = np.array(str(err))
      with open(path) as f:
        files[name] = f.read()
      out['write/{}/text'.format(tag)] = np.array(files[name])
  np.savez_compressed(OUT, **out)
  print('wrote', OUT, os.path.getsize(OUT), 'bytes;', len(out), 'entries')
  for e in range(len(C.ENVS)):
    print('env', e, 'bounds', out['run{}/episode_bounds'.format(e)], 'return', out['analyse{}/return'.format(e)])
    print(out['analyse{}/corrcoef'.format(e)], out['analyse{}/overlap_std'.format(e)], sep='\n')


if __name__ == '__main__':
  main()
