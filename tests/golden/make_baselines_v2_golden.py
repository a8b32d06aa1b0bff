#!/usr/bin/env python3
"""Golden vectors for the heuristic baselines on Stack-v2 observations (one overhead map, G object maps per env) from the
reference's own `stackrl/baselines.py` and `stackrl/agents/policies.py`: `Baseline(method, value=True, batched=True,
batchwise=True)`, the policy `python -m stackrl test` builds for a four-dimensional observation (`__main__.py:111-117`).

Runs only in the build container.  Both modules are loaded by file path.  Their headers import gin, gym and TensorFlow,
none of which is installed and none of which the code exercised here computes with: the placeholders are a no-op
`gin.configurable`, an empty `gym`, and a `tf` whose `nest.flatten` / `nest.pack_sequence_as` handle the 2-tuple
observation, which is all `PyGreedy.__call__` (policies.py:57-91) asks of it.

The file written (`baselines_v2_golden.npz`) holds arrays and short labels only: the observations in the vectorised env's
layout (maps [B, H, H, 2], object maps [B, G, h, h, 1]; the reference gets the map stacked G times, env.py:472-480), and per
method x goal x minorder the reference's (row, action) per env and every row's returned value at its own action; for one
configuration per method the returned maps; the row a plain arg-min over all rows' raw values would take.  It is written
with fixed zip timestamps, so that the script reproduces it byte for byte."""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

REF_DIR = '/root/reference/stackrl'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'baselines_v2_golden.npz')
METHODS = ('height', 'difference', 'corrcoef', 'correlate')
GOALS = (True, False)
MINORDERS = (0, 1)
MAPS_CONFIG = (True, 1)                  # (goal, minorder) of the configuration whose returned maps are recorded
SHAPES = (('s32', 32, 8, 4, 6), ('s64', 64, 16, 8, 2))     # tag, H, h, G, envs
SEED0 = 1


def _load(name, path):
  spec = importlib.util.spec_from_file_location(name, path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def load_reference():
  sys.dont_write_bytecode = True   # the reference tree is read-only: no __pycache__ beside its files
  gin = types.ModuleType('gin')
  gin.configurable = lambda *a, **k: (lambda f: f) if not (len(a) == 1 and callable(a[0])) else a[0]
  gym = types.ModuleType('gym')
  tf = types.ModuleType('tensorflow')
  tf.Module = object
  tf.nest = types.SimpleNamespace(flatten=lambda s: list(s), pack_sequence_as=lambda s, flat: tuple(flat))
  stackrl = types.ModuleType('stackrl')
  names = ('gin', 'gym', 'tensorflow', 'stackrl', 'stackrl.agents')
  saved = {k: sys.modules.get(k) for k in names}
  sys.modules.update({'gin': gin, 'gym': gym, 'tensorflow': tf, 'stackrl': stackrl})
  try:
    agents = types.ModuleType('stackrl.agents')
    agents.PyGreedy = _load('ref_policies', os.path.join(REF_DIR, 'agents', 'policies.py')).PyGreedy
    stackrl.agents = agents
    sys.modules['stackrl.agents'] = agents
    mod = _load('ref_baselines', os.path.join(REF_DIR, 'baselines.py'))
  finally:
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v
  return mod


def make_rock(rng, h):
  """An off-centre half-ellipsoid with a ridge: its 90-degree turns are different object maps."""
  a, b = rng.randint(h // 2, h - 1), rng.randint(h // 3, h // 2 + 1)
  top, low = rng.randint(50, 120), rng.randint(15, 40)
  yy, xx = np.mgrid[0:a, 0:b]
  r2 = ((yy - a / 2 + 0.5) / (a / 2)) ** 2 + ((xx - b / 2 + 0.5) / (b / 2)) ** 2
  rock = np.where(r2 <= 1, low + (top - low) * np.clip(1 - r2, 0, 1) * (0.5 + 0.5 * yy / a), 0).astype(np.uint8)
  o = np.zeros((h, h), np.uint8)
  u, v = rng.randint(0, h - a + 1), rng.randint(0, h - b + 1)
  o[u:u + a, v:v + b] = rock
  return o


def make_env(rng, H, h, G):
  """One env: a goal rectangle, a pile that covers it (so that the lowest spot of the map is not inside the goal) and bare
  ground around it; G object maps: G / turns rocks, each in `turns` 90-degree turns."""
  m = np.zeros((H, H, 2), np.uint8)
  gu, gv = rng.randint(H // 16, H // 4, 2)
  gh, gw = rng.randint(H // 3, H // 2 + 1, 2)
  m[gu:gu + gh, gv:gv + gw, 1] = rng.randint(120, 256)
  for _ in range(rng.randint(3, 7)):
    a, b = rng.randint(H // 8, H // 3, 2)
    u, v = gu + rng.randint(-a // 2, gh - a // 2), gv + rng.randint(-b // 2, gw - b // 2)
    u, v = int(np.clip(u, 0, H - a)), int(np.clip(v, 0, H - b))
    yy, xx = np.mgrid[0:a, 0:b]
    blob = (rng.randint(20, 110) * np.clip(1 - ((yy - a / 2) / (a / 2)) ** 2 - ((xx - b / 2) / (b / 2)) ** 2, 0, 1)).astype(np.uint8)
    m[u:u + a, v:v + b, 0] = np.maximum(m[u:u + a, v:v + b, 0], blob)
  step = H // 8                                            # the pile's base: rough blocks of uneven height all over the goal
  base = (np.kron(rng.randint(15, 70, (8, 8)), np.ones((step, step), np.int64)) + rng.randint(0, 16, (H, H))).astype(np.uint8)
  inside = m[:, :, 1] > 0
  m[:, :, 0] = np.where(inside, np.maximum(m[:, :, 0], base), m[:, :, 0])
  turns = 2 if G == 4 else 4
  rows = []
  for _ in range(G // turns):
    rock = make_rock(rng, h)
    rows += [np.rot90(rock, k).copy() for k in range(turns)]
  return m, np.stack(rows)[..., None]


def record(ref, seed):
  """The fixture's arrays from one seed, and the share of (env, method, minorder) cases with goal=True whose row differs
  from the plain arg-min's."""
  rng = np.random.RandomState(seed)
  out = {'methods': np.array(METHODS), 'shapes': np.array([s[0] for s in SHAPES]), 'minorders': np.array(MINORDERS, np.int64),
         'maps_config': np.array([int(MAPS_CONFIG[0]), MAPS_CONFIG[1]], np.int64), 'seed': np.int64(seed)}
  differ = total = 0

  def rec(key, x):
    x = np.asarray(x)
    assert np.all(np.isfinite(x)), key
    out[key] = x

  for tag, H, h, G, n_env in SHAPES:
    envs = [make_env(rng, H, h, G) for _ in range(n_env)]
    rec(tag + '/obs_map', np.stack([m for m, _ in envs]))
    rec(tag + '/obs_obj', np.stack([o for _, o in envs]))
    for method in METHODS:
      plain = []
      for m, o in envs:    # what OrientationGreedy(minimize=True) over the raw values takes: the row of the overall minimum
        raw = np.stack([np.asarray(ref.methods[method]((m.copy(), o[r].copy())), dtype=np.float64).ravel() for r in range(G)])
        plain.append(int(np.argmin(raw.ravel())) // raw.shape[1])
      rec('{}/{}/plain_row'.format(tag, method), np.array(plain, np.int64))
      for goal in GOALS:
        for mo in MINORDERS:
          pol = ref.Baseline(method=method, goal=goal, minorder=mo, value=True, batched=True, batchwise=True)
          rows, acts, cs, maps = [], [], [], []
          for m, o in envs:
            inp = (np.stack([m] * G), o.copy())            # env.py:472-480: the overhead map once per object map
            (row, act), vals = pol(inp)
            c = []
            for r in range(G):                             # each row's own (action, returned map): Baseline.call
              a_r, neg_r = pol.call((m.copy(), o[r].copy()))
              assert np.array_equal(np.asarray(neg_r).ravel(), vals[r])
              c.append(float(np.asarray(neg_r).ravel()[a_r]))
            assert int(row) == int(np.argmax(c)) and c[int(row)] == vals[int(row)][int(act)]
            rows.append(int(row)); acts.append(int(act)); cs.append(c); maps.append(np.asarray(vals, dtype=np.float64))
          key = '{}/{}/g{}_m{}'.format(tag, method, int(goal), mo)
          rec(key + '/row', np.array(rows, np.int64))
          rec(key + '/action', np.array(acts, np.int64))
          rec(key + '/c', np.array(cs, np.float64))
          if (goal, mo) == MAPS_CONFIG:
            rec(key + '/maps', np.stack(maps))             # [envs, G, A]
          if goal:
            differ += int(np.sum(np.array(rows) != np.array(plain))); total += n_env
  return out, differ, total


def write_npz(path, arrays):
  """np.savez_compressed with the zip members' timestamps fixed: the same arrays give the same bytes."""
  with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
    for k in sorted(arrays):
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
      info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
  ref = load_reference()
  seed = SEED0
  while True:     # seeds in order until the reference alone tells this policy from the plain arg-min in a third of the cases
    out, differ, total = record(ref, seed)
    print('seed {}: the reference row differs from the plain arg-min row in {} of {} goal=True cases'.format(seed, differ, total))
    if 3 * differ >= total:
      break
    seed += 1
  write_npz(OUT, out)
  size = os.path.getsize(OUT)
  assert size < 300 * 1024, size
  print('wrote', OUT, size, 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
  main()
