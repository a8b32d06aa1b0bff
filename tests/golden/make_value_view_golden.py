#!/usr/bin/env python3
"""Writes tests/golden/value_view_golden.npz with matplotlib (CPU only): the colour table of `viridis` and, for a set of tiny
float32 maps, the bytes matplotlib draws them with — `ax.imshow(v)` as the reference's visualised run calls it
(stackrl/test.py:304: default norm, default colour map), then `im.to_rgba(im.get_array(), bytes=True)`.  A cell imshow masks
(NaN, +-inf) comes out with alpha 0: the figure's background shows there.

  lut        uint8 [256, 3]   (uint8)(viridis * 255): what `cmap(..., bytes=True)` indexes
  lut_round  uint8 [256, 3]   (uint8)(viridis * 255 + 0.5): the table of the wrong variant 'lut_round'
  maps       float32 [M, 9, 9]
  rgba       uint8 [M, 9, 9, 4]
  names      [M]

The maps are 9 x 9 so that they drop into the value maps of a 16 / 8 env.  The spans of the 'searched' maps were found here, by
search, as the first on which a wrong variant of tests/value_view_cases.py differs from matplotlib."""
import os
import sys

import matplotlib
matplotlib.use('Agg')
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
from matplotlib import cm  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import value_view_cases as cases  # noqa: E402

N = 9
F32 = np.float32


def drawn(v, ax):
  ax.cla()
  im = ax.imshow(v)
  if not np.isfinite(v).any():                 # nothing to scale by: every cell is masked
    return np.zeros(v.shape + (4,), np.uint8)
  return im.to_rgba(im.get_array(), bytes=True)


def edges(vmin, span, rng):
  """81 of the 257 bin edges vmin + k span / 256, both ends among them, in float32."""
  k = np.concatenate([[0, 256], rng.choice(np.arange(1, 256), N * N - 2, replace=False)])
  rng.shuffle(k)
  return (F32(vmin) + k.astype(F32) * F32(span) / F32(256)).astype(F32).reshape(N, N)


def main():
  rng = np.random.RandomState(20)
  colors = np.array(cm.viridis.colors, dtype=np.float64)
  lut = (colors * 255).astype(np.uint8)
  assert np.array_equal(lut, cm.viridis(np.arange(256), bytes=True)[:, :3])
  cases._golden = {'lut': lut, 'lut_round': (colors * 255 + 0.5).astype(np.uint8)}
  _, ax = plt.subplots()
  maps, names = [], []

  def add(name, v):
    names.append(name)
    maps.append(np.asarray(v, F32).reshape(N, N))

  for e in (-6, -2, 0, 4, 30):
    add('random 1e{}'.format(e), rng.standard_normal((N, N)) * 10.0 ** e + rng.standard_normal() * 10.0 ** e)
  add('random uniform', rng.uniform(0, 1, (N, N)))
  add('constant', np.full((N, N), 1.25))
  add('constant zero', np.zeros((N, N)))
  v = rng.standard_normal((N, N))
  v[0, 0], v[3, 4], v[8, 8] = np.nan, np.inf, -np.inf
  add('nan and infinities', v)
  v = rng.standard_normal((N, N))
  top, bottom = np.unravel_index(v.argmax(), v.shape), np.unravel_index(v.argmin(), v.shape)
  v[top], v[bottom] = np.nan, -np.inf                        # the would-be extremes are not finite
  v[1, 1] = np.inf
  add('non-finite at the extremes', v)
  v = np.full((N, N), np.nan)
  v[4, 4] = 2.0
  add('one finite cell', v)
  v = np.full((N, N), np.nan)
  v[::2] = np.inf
  v[1, 1] = -np.inf
  add('all non-finite', v)
  v = rng.standard_normal((N, N))
  v[v > 0.3] = 0.3
  add('tied maxima', v)
  for vmin, span in ((0.0, 0.1), (0.0, 3.0), (0.0, 7.0), (-1.7, 0.1), (2.5, 3.0), (100.0, 7.0), (-0.3, 1.0)):
    add('bin edges vmin {} span {}'.format(vmin, span), edges(vmin, span, rng))
  # a span on which each cell-level wrong variant differs from matplotlib: the first of a seeded search
  for variant in cases.CELL_VARIANTS:
    have = [m for m in maps if not np.array_equal(cases.colour_cells(m, variant)[np.isfinite(m)], drawn(m, ax)[..., :3][np.isfinite(m)])]
    if have:
      continue
    for trial in range(100000):
      vmin, span = rng.uniform(-4, 4), 10.0 ** rng.uniform(-2, 2)
      v = edges(vmin, span, rng)
      if not np.array_equal(cases.colour_cells(v, variant), drawn(v, ax)[..., :3]):
        add('searched for {}: bin edges vmin {!r} span {!r}'.format(variant, vmin, span), v)
        break
    else:
      raise SystemExit('no map found on which {} differs'.format(variant))
  maps = np.stack(maps)
  rgba = np.stack([drawn(v, ax) for v in maps])
  # the definition gives these bytes (finite cells), and alpha is 0 exactly where the cell is not finite
  for name, v, img in zip(names, maps, rgba):
    fin = np.isfinite(v)
    assert np.array_equal(img[..., 3] == 255, fin) and np.array_equal(img[..., 3] == 0, ~fin), name
    assert np.array_equal(cases.colour_cells(v)[fin], img[..., :3][fin]), name
  out = os.path.join(HERE, 'value_view_golden.npz')
  np.savez_compressed(out, lut=lut, lut_round=cases._golden['lut_round'], maps=maps, rgba=rgba, names=np.array(names))
  print(out, os.path.getsize(out), 'bytes,', len(names), 'maps')
  for n in names:
    print(' ', n)


if __name__ == '__main__':
  main()
