#!/usr/bin/env python3
"""Golden vectors for the heuristic baseline policies from the reference's own `stackrl/baselines.py`.

Runs only in the build container.  baselines.py is numpy/scipy code, but its module header imports gin, gym and
`stackrl.agents` (TensorFlow), none of which is installed.  The functions exercised here (`height`, `difference`,
`corrcoef`, `correlate`, `goal_overlap`, `Baseline.call`) use none of those imports, so the module is loaded by file
path with inert placeholders for the three names (a no-op `gin.configurable`, an empty `gym`, a `PyGreedy` base
class that only forwards `__call__` to `call`).  Inputs are seeded uint8 observations in the env's format; the file
written (`baselines_golden.npz`) holds inputs and expected outputs only.  A second file (`baselines_edges_golden.npz`)
holds small observations (H <= 64) at the edges of the kernels' paths: other map sizes, per-observation goal maxima, the
zero-variance branches of `corrcoef`, thin and one-pixel objects, the `pow` exponents of `difference`, four mask
thresholds and the selection at minorder 0-3.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = '/root/reference/stackrl/baselines.py'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'baselines_golden.npz')
OUT_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'baselines_edges_golden.npz')


def load_reference():
  sys.dont_write_bytecode = True   # the reference tree is read-only: no __pycache__ beside its files
  gin = types.ModuleType('gin')
  gin.configurable = lambda *a, **k: (lambda f: f) if not (len(a) == 1 and callable(a[0])) else a[0]
  gym = types.ModuleType('gym')
  stackrl = types.ModuleType('stackrl')
  agents = types.ModuleType('stackrl.agents')

  class PyGreedy(object):
    def __call__(self, inputs):
      return self.call(inputs)
  agents.PyGreedy = PyGreedy
  stackrl.agents = agents
  saved = {k: sys.modules.get(k) for k in ('gin', 'gym', 'stackrl', 'stackrl.agents')}
  sys.modules.update({'gin': gin, 'gym': gym, 'stackrl': stackrl, 'stackrl.agents': agents})
  try:
    spec = importlib.util.spec_from_file_location('ref_baselines', REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
  finally:
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v
  return mod


def make_obs(rng, H=128, h=32, goal=170):
  """A plausible observation: blobs of height on the map, a goal rectangle, a rock-shaped object map.  The sizes are
  those of the 128 / 32 observation scaled by H / 128 (the same draws and the same arrays at H = 128)."""
  def q(x):
    return max(1, x * H // 128)
  m = np.zeros((H, H, 2), np.uint8)
  for _ in range(rng.randint(0, 6)):
    u, v = rng.randint(0, H - q(30), 2); a, b = rng.randint(q(8), max(q(8) + 1, q(30)), 2)
    yy, xx = np.mgrid[0:a, 0:b]
    blob = (rng.randint(20, 90) * np.clip(1 - ((yy - a / 2) / (a / 2)) ** 2 - ((xx - b / 2) / (b / 2)) ** 2, 0, 1)).astype(np.uint8)
    m[u:u + a, v:v + b, 0] = np.maximum(m[u:u + a, v:v + b, 0], blob)
  gu, gv = rng.randint(q(8), q(40), 2); gh, gw = rng.randint(q(32), q(80)), rng.randint(q(32), q(80))
  m[gu:gu + gh, gv:gv + gw, 1] = goal
  o = np.zeros((h, h, 1), np.uint8)
  a, b = rng.randint(h // 3, h - 4, 2)
  yy, xx = np.mgrid[0:a, 0:b]
  rock = (60 - 35 * np.clip(1 - ((yy - a / 2) / (a / 2)) ** 2 - ((xx - b / 2) / (b / 2)) ** 2, 0, 1))
  rock = np.where(((yy - a / 2) / (a / 2)) ** 2 + ((xx - b / 2) / (b / 2)) ** 2 <= 1, rock, 0).astype(np.uint8)
  o[(h - a) // 2:(h - a) // 2 + a, (h - b) // 2:(h - b) // 2 + b, 0] = rock
  return m, o


CASES = [('height', 'height', {}), ('difference', 'difference', {}),
         ('difference_e1w0', 'difference', dict(difference_exponent=1, weights_exponent=0)),
         ('corrcoef', 'corrcoef', {}), ('corrcoef_localized', 'corrcoef', dict(localized=True)),
         ('correlate', 'correlate', {})]
POW_CASES = [('difference_e{}w{}'.format(e, w), 'difference', dict(difference_exponent=e, weights_exponent=w))
             for e, w in ((3, 1), (1, 3), (2, 4))]     # the exponents that go through pow on both sides
THRESHOLDS = (1.0, 0.75, 0.5, 0.0)
SELECT_METHODS = ('height', 'difference', 'corrcoef', 'correlate')


def edge_observations():
  """name -> (map uint8 [H, H, 2], object uint8 [h, h, 1]).  Observations of one shape carry different goal values, so
  that a batch stacked from them has a different goal maximum (`get_inputs`, baselines.py:23) in every env."""
  rng = np.random.RandomState(23)
  obs = {}
  # the other map sizes: resolution factors 4 and 3, two observable size ratios, one window, four windows
  for H, h, goal in ((64, 16, 170), (64, 16, 9), (32, 8, 170), (48, 16, 170), (40, 32, 170), (16, 16, 170), (16, 16, 255),
                     (33, 32, 170), (33, 32, 3)):
    obs['shape_{}_{}_g{}'.format(H, h, goal)] = make_obs(rng, H, h, goal)
  obs['goal255_32_8'] = make_obs(rng, 32, 8, 255)
  obs['goal1_32_8'] = make_obs(rng, 32, 8, 1)
  m, _ = make_obs(rng, 32, 8, 200)                                     # n_var == 0 (baselines.py:97)
  obs['constant_object_32_8'] = (m, np.full((8, 8, 1), 37, np.uint8))
  m, o = make_obs(rng, 48, 16, 99)                                     # o_var == 0 (baselines.py:111) on bare ground and,
  m[:, :, 0] = 0                                                       # up to its own rounding, on the plateau
  m[6:38, 9:41, 0] = 57
  m[40:46, 2:8, 0] = np.arange(36, dtype=np.uint8).reshape(6, 6) + 10
  obs['plateau_48_16'] = (m, o)
  m, o = make_obs(rng, 40, 32, 211)
  m[:, :, 0] = 83
  m[0:3, 0:3, 0] = 0
  obs['plateau_40_32'] = (m, o)
  m, _ = make_obs(rng, 48, 16, 131)                                    # 20 of 256 pixels: a thin diagonal and a short bar
  o = np.zeros((16, 16, 1), np.uint8)
  o[np.arange(2, 14), np.arange(1, 13), 0] = 30 + 3 * np.arange(12, dtype=np.uint8)
  o[12, 2:10, 0] = 45
  assert np.count_nonzero(o) < 0.1 * o.size
  obs['sparse_object_48_16'] = (m, o)
  m, _ = make_obs(rng, 32, 8, 77)                                      # one tap, off the centre (its `difference` weight is
  o = np.zeros((8, 8, 1), np.uint8)                                    # the distance from the centre)
  o[2, 5, 0] = 41
  obs['one_pixel_object_32_8'] = (m, o)
  return obs


def edges(ref):
  """Inputs at the edges of the kernels' paths and what the reference returns on them (no input on which the reference
  itself yields NaN: every recorded array is checked to be finite)."""
  out = {}
  obs = edge_observations()
  out['names'] = np.array(sorted(obs))
  for name in sorted(obs):
    m, o = obs[name]
    def rec(key, x):
      x = np.asarray(x)
      assert np.all(np.isfinite(x)), (name, key)
      out[name + '/' + key] = x
    rec('map', m); rec('obj', o)
    for tag, fn, kw in CASES + POW_CASES:
      rec(tag, np.asarray(getattr(ref, fn)((m.copy(), o.copy()), **kw), dtype=np.float64))
    for t in THRESHOLDS:
      rec('goal_overlap_t{:03d}'.format(int(100 * t)), ref.goal_overlap((m, o), threshold=t))
    for method in SELECT_METHODS:
      for minorder in (0, 1, 2, 3):
        a, v = ref.Baseline(method=method, goal=True, minorder=minorder, threshold=1.0)((m.copy(), o.copy()))
        rec('select_{}_g1_m{}_action'.format(method, minorder), np.int64(a))
        key = name + '/select_{}_g1_values'.format(method)            # the returned map does not depend on minorder
        if minorder == 0:
          rec('select_{}_g1_values'.format(method), np.asarray(v, dtype=np.float64))
        else:
          assert np.array_equal(out[key], v)
        a, v = ref.Baseline(method=method, goal=False, minorder=minorder, threshold=1.0)((m.copy(), o.copy()))
        rec('select_{}_g0_m{}_action'.format(method, minorder), np.int64(a))
        assert np.array_equal(v, -out[name + '/' + method])            # goal=False returns -values: not stored
  return out


def main():
  ref = load_reference()
  rng = np.random.RandomState(11)
  out = {}
  n_case = 5
  maps, objs = zip(*[make_obs(rng) for _ in range(n_case)])
  out['obs_map'] = np.stack(maps); out['obs_obj'] = np.stack(objs)
  for name, fn, kw in CASES:
    out[name] = np.stack([np.asarray(getattr(ref, fn)((m.copy(), o.copy()), **kw), dtype=np.float64) for m, o in zip(maps, objs)])
  out['goal_overlap'] = np.stack([ref.goal_overlap((m, o)) for m, o in zip(maps, objs)])
  for method in ('height', 'difference', 'corrcoef', 'correlate'):
    for goal, minorder in ((True, 1), (True, 0), (False, 1)):
      pol = ref.Baseline(method=method, goal=goal, minorder=minorder)
      acts, vals = zip(*[pol((m.copy(), o.copy())) for m, o in zip(maps, objs)])
      tag = 'select_{}_g{}_m{}'.format(method, int(goal), minorder)
      out[tag + '_action'] = np.array(acts, dtype=np.int64)
      out[tag + '_values'] = np.stack([np.asarray(v, dtype=np.float64) for v in vals])
  np.savez_compressed(OUT, **out)
  print('wrote', OUT, os.path.getsize(OUT), 'bytes;', {k: v.shape for k, v in out.items() if not k.startswith('select')})
  out = edges(ref)
  np.savez_compressed(OUT_EDGES, **out)
  print('wrote', OUT_EDGES, os.path.getsize(OUT_EDGES), 'bytes;', len(out['names']), 'observations,', len(out), 'arrays')


if __name__ == '__main__':
  main()
