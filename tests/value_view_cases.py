"""The definition of include/stackrl_valueview.h restated in numpy (`reference_frames`), the named wrong variants the tests
must tell from it, and the synthetic inputs the CPU and GPU suites share.

The colour table is matplotlib's, read from tests/golden/value_view_golden.npz (made by tests/golden/make_value_view_golden.py),
not from the library: tests/test_valueview_abi.py holds the library's table to the same file."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'value_view_golden.npz')
GAP, BORDER, MAX_SHOWN, PER_LINE = 8, 3, 6, 3
BACKGROUND = np.array([255, 255, 255], np.uint8)
RED = np.array([255, 0, 0], np.uint8)
F32 = np.float32

# the wrong variants: what each does instead of the definition
VARIANTS = {
  'float64': 'the normalisation in float64',
  'reciprocal': 'multiplies by a float32 reciprocal of the span instead of dividing',
  'rint255': 'rint(t * 255) instead of truncating t * 256',
  'all_cells': 'vmin and vmax over all cells instead of the finite ones',
  'lut_round': 'the table as viridis * 255 + 0.5',
  'window_noclip': 'the window without the clip',
  'ring_tile_index': 'the ring on tile `index` instead of the tile that shows policy `index`',
}
CELL_VARIANTS = ('float64', 'reciprocal', 'rint255', 'all_cells', 'lut_round')

_golden = None


def golden():
  global _golden
  if _golden is None:
    with np.load(GOLDEN) as z:
      _golden = {k: z[k] for k in z.files}
  return _golden


# ---------------------------------------------------------------------------------------------------- layout and window
def layout(H, h, P, s):
  """The closed forms of section 4 as a dict (integers)."""
  OH = H - h + 1
  nv = min(P, MAX_SHOWN)
  ncol, nline = min(nv, PER_LINE), 1 + (nv > PER_LINE)
  SH, Sh, TB = s * H, s * h, s * OH + 2 * BORDER
  return dict(OH=OH, nv=nv, ncol=ncol, nline=nline, SH=SH, Sh=Sh, ST=s * OH, TB=TB,
              FW=2 * GAP + SH + ncol * (TB + GAP), FH=max(3 * GAP + SH + Sh, GAP + nline * (TB + GAP)))


def window(P, index, variant=None):
  nv = min(P, MAX_SHOWN)
  if variant == 'window_noclip':
    return index - nv // 2
  return int(np.clip(index - nv // 2, 0, P - nv))


def regions(H, h, P, s):
  """name -> (row0, row1, col0, col1), half open: the two views and the boxes of the tiles."""
  l = layout(H, h, P, s)
  out = {'overhead': (GAP, GAP + l['SH'], GAP, GAP + l['SH']),
         'object': (2 * GAP + l['SH'], 2 * GAP + l['SH'] + l['Sh'], GAP, GAP + l['Sh'])}
  for k in range(l['nv']):
    r0 = GAP + (k // PER_LINE) * (l['TB'] + GAP)
    c0 = 2 * GAP + l['SH'] + (k % PER_LINE) * (l['TB'] + GAP)
    out['tile{}'.format(k)] = (r0, r0 + l['TB'], c0, c0 + l['TB'])
  return out


# ---------------------------------------------------------------------------------------------------- the colour of a cell
def colour_cells(x, variant=None):
  """uint8 [..., 3] of a map x (any shape; rounded to float32 first): section 2, or one of `CELL_VARIANTS`."""
  g = golden()
  lut = g['lut_round'] if variant == 'lut_round' else g['lut']
  with np.errstate(all='ignore'):
    x = np.asarray(x).astype(F32)
    out = np.empty(x.shape + (3,), np.uint8)
    out[...] = BACKGROUND
    fin = np.isfinite(x)
    if variant == 'all_cells':
      vmin, vmax = x.min(), x.max()
    elif fin.any():
      vmin, vmax = x[fin].min(), x[fin].max()
    else:
      return out
    if not vmin <= vmax:
      return out
    if variant == 'float64':
      t = (x.astype(np.float64) - np.float64(vmin)) / (np.float64(vmax) - np.float64(vmin))
    elif variant == 'reciprocal':
      t = (x - vmin) * (F32(1) / (vmax - vmin))
    else:
      t = x - vmin
      t = t / (vmax - vmin)
    if variant == 'rint255':
      t = np.rint(t * t.dtype.type(255))
    else:
      t = t * t.dtype.type(256)
    if vmax == vmin:
      t = np.zeros_like(t)
    k = np.where(t > 0, np.where(t >= 255, 255, np.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0)), 0).astype(np.int32)
    out[fin] = lut[k[fin]]
  return out


# ---------------------------------------------------------------------------------------------------- the frames
def chosen(values, actions, j, b, A):
  """(the chosen row's map of policy j in env b, float32 [A]; its pixel or None)."""
  v = np.asarray(values[j])
  v = v.reshape(v.shape[0], -1, A)
  if actions is None:
    return v[b, 0].astype(F32), None
  a = int(np.asarray(actions)[j][b])
  return v[b, int(np.clip(a // A, 0, v.shape[1] - 1))].astype(F32), a % A


def _blocks(img, s):
  return np.repeat(np.repeat(img, s, axis=0), s, axis=1)


def reference_frames(rgb0, rgb1, values, actions=None, index=0, indexes=None, scale=2, mark=False, variant=None):
  """uint8 [n, FH, FW, 3].  rgb0 uint8 [B, H, H, 3], rgb1 uint8 [B, h, h, 3]; values: P arrays [B, G * A] / [B, G, A] of a float
  type; actions: None or int [P, B]; indexes: the envs of the frames (default all, in order)."""
  rgb0, rgb1 = np.asarray(rgb0), np.asarray(rgb1)
  B, H, h, P, s = rgb0.shape[0], rgb0.shape[1], rgb1.shape[1], len(values), int(scale)
  l = layout(H, h, P, s)
  OH, A = l['OH'], l['OH'] ** 2
  indexes = np.arange(B) if indexes is None else np.clip(np.asarray(indexes), 0, B - 1)
  reg = regions(H, h, P, s)
  min_j = window(P, index, variant)
  ring_colour = golden()['lut'][255]
  frames = np.empty((len(indexes), l['FH'], l['FW'], 3), np.uint8)
  frames[...] = BACKGROUND
  for f, b in enumerate(indexes):
    over = rgb0[b].copy()
    if mark and actions is not None:
      u, v = divmod(chosen(values, actions, index, b, A)[1], OH)
      win = over[u:u + h, v:v + h]
      win[0], win[-1], win[:, 0], win[:, -1] = RED, RED, RED, RED
    r0, r1, c0, c1 = reg['overhead']
    frames[f, r0:r1, c0:c1] = _blocks(over, s)
    r0, r1, c0, c1 = reg['object']
    frames[f, r0:r1, c0:c1] = _blocks(rgb1[b], s)
    for k in range(l['nv']):
      j = min_j + k
      if not 0 <= j < P:
        continue                                    # (only a wrong window gets here)
      r0, r1, c0, c1 = reg['tile{}'.format(k)]
      if (k == index) if variant == 'ring_tile_index' else (j == index):
        frames[f, r0:r1, c0:c1] = ring_colour
      x, pixel = chosen(values, actions, j, b, A)
      cells = colour_cells(x, variant if variant in CELL_VARIANTS else None)
      if mark and pixel is not None:
        cells[pixel] = RED
      frames[f, r0 + BORDER:r1 - BORDER, c0 + BORDER:c1 - BORDER] = _blocks(cells.reshape(OH, OH, 3), s)
  return frames


# ---------------------------------------------------------------------------------------------------- synthetic inputs
def synthetic(B, H, h, P, G=1, f64_mask=0, seed=0, with_actions=True, corners=False, wide=False):
  """(rgb0, rgb1, values, actions): random images, smooth-plus-noise maps of different magnitudes per policy (float64 where
  bit j of f64_mask is set), and actions that choose different rows per env and policy.  `corners`: the pixels of the first
  envs and policies go through the four corners of the action map.  `wide`: the actions of policy 0 lie beyond 2^33 (their row
  clamps to the last) and those of policy 1 are negative (row 0), with the pixels they had."""
  rng = np.random.RandomState(seed)
  OH = H - h + 1
  A = OH * OH
  rgb0 = rng.randint(0, 256, (B, H, H, 3)).astype(np.uint8)
  rgb1 = rng.randint(0, 256, (B, h, h, 3)).astype(np.uint8)
  values = []
  for j in range(P):
    v = rng.standard_normal((B, G, A)) * 10.0 ** rng.randint(-3, 4) + rng.standard_normal((B, G, 1))
    values.append(v.astype(np.float64 if (f64_mask >> j) & 1 else np.float32))
  actions = None
  if with_actions:
    rows = (np.arange(P)[:, None] + 2 * np.arange(B)[None, :] + 1) % G
    pixels = rng.randint(0, A, (P, B))
    if corners:
      corner = np.array([0, OH - 1, A - OH, A - 1])
      pixels = corner[(np.arange(P)[:, None] + np.arange(B)[None, :]) % 4]
    actions = (rows * A + pixels).astype(np.int64)
    if wide:
      actions[0] += A * 2 ** 33
      actions[1 % P] -= A * 5
  return rgb0, rgb1, values, actions


def fixture_inputs():
  """The committed maps as the value maps of a 16 / 8 env (A = 81), one env per map: policy 0 holds them in float32, policy 1
  in float64 and in reverse order.  (rgb0, rgb1, values, None)."""
  maps = golden()['maps']
  B = len(maps)
  rgb0, rgb1, _, _ = synthetic(B, 16, 8, 1, seed=9, with_actions=False)
  flat = maps.reshape(B, 1, 81)
  return rgb0, rgb1, [flat.copy(), flat[::-1].astype(np.float64)], None


def _case(tag, H, h, P, s, B=2, G=1, f64_mask=0, index=0, indexes=None, mark=False, with_actions=True, corners=False, seed=0,
          wide=False):
  return tag, dict(H=H, h=h, P=P, scale=s, B=B, G=G, f64_mask=f64_mask, index=index, indexes=indexes, mark=mark,
                   with_actions=with_actions, corners=corners, seed=seed, wide=wide)


def device_cases():
  """(tag, parameters) of every synthetic case the GPU suite draws; `case_inputs` makes the arrays.  16 / 8: A = 81, less than
  two waves and no multiple of 64; 32 / 8: A = 625; 128 / 32: A = 9,409, several waves per reduction; 17 / 8: frames whose size
  leaves 3 and 1 bytes beyond the last whole word."""
  out = [_case('16/8 s{} P3'.format(s), 16, 8, 3, s, index=1, seed=s) for s in (1, 2, 3)]
  out += [_case('16/8 P8 index {}'.format(i), 16, 8, 8, 1, B=2, G=2, index=i, mark=True, f64_mask=0b10100101, seed=10 + i)
          for i in range(8)]
  out += [
    _case('16/8 P1 no actions', 16, 8, 1, 2, with_actions=False, seed=20),
    _case('16/8 P4 corners marked', 16, 8, 4, 3, B=4, index=2, mark=True, corners=True, seed=21),
    _case('16/8 P6 corners marked G4 f64', 16, 8, 6, 2, B=4, G=4, index=5, mark=True, corners=True, f64_mask=0b111111, seed=22),
    _case('16/8 B5 indexes 4 0 4', 16, 8, 3, 2, B=5, G=4, indexes=[4, 0, 4], index=2, f64_mask=0b010, mark=True, seed=23),
    _case('16/8 indexes clamped', 16, 8, 2, 1, B=3, indexes=[-3, 99, 1], seed=24),
    _case('16/8 actions beyond 32 bits and negative', 16, 8, 3, 2, B=3, G=4, index=1, mark=True, wide=True, seed=33),
    _case('17/8 P1 tail 3', 17, 8, 1, 1, B=1, seed=25),
    _case('17/8 P1 tail 1', 17, 8, 1, 1, B=3, mark=True, seed=26),
    _case('32/8 P4 s3 odd', 32, 8, 4, 3, B=3, G=4, index=3, f64_mask=0b0101, mark=True, seed=27),
    _case('32/8 P6 s1 odd', 32, 8, 6, 1, B=1, index=0, seed=28),
    _case('32/8 P3 s2', 32, 8, 3, 2, B=2, G=1, index=0, mark=False, seed=29),
    _case('128/32 P6 s1', 128, 32, 6, 1, B=2, index=4, f64_mask=0b001000, mark=True, seed=30),
    _case('128/32 P4 s2 G4', 128, 32, 4, 2, B=2, G=4, indexes=[1], index=1, f64_mask=0b0011, seed=31),
    _case('128/32 P1 s3', 128, 32, 1, 3, B=1, mark=True, seed=32),
  ]
  return out


def case_inputs(p):
  """(rgb0, rgb1, values, actions) of the parameters of a `device_cases` entry."""
  return synthetic(p['B'], p['H'], p['h'], p['P'], G=p['G'], f64_mask=p['f64_mask'], seed=p['seed'],
                   with_actions=p['with_actions'], corners=p['corners'], wide=p['wide'])


def case_frames(p, inputs, variant=None):
  rgb0, rgb1, values, actions = inputs
  return reference_frames(rgb0, rgb1, values, actions, index=p['index'], indexes=p['indexes'], scale=p['scale'], mark=p['mark'],
                          variant=variant)
