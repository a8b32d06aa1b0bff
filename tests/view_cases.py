"""`StackEnv.render('rgb_array')` (env.py:299-311; `TestStackEnv.render`, :562-575) restated in numpy, the wrong variants the
tests must tell apart from it, and the selection of the object map the reference renders from `VecStackEnv.maps()`."""
import numpy as np


def _colour(m, goal_rect=None):
  """One map float32 [H, W] -> float64 [H, W, 3], as env.py:299-305 writes it."""
  m = np.asarray(m)
  assert m.dtype == np.float32 and m.ndim == 2
  _max = np.max(m)
  r = m / _max if _max != 0 else m          # float32 / float32
  b = 1 - r                                 # float32
  g = np.ones(r.shape) * 0.5                # float64
  if goal_rect is not None:
    u, v, h, w = (int(x) for x in goal_rect)
    g[u:u + h, v:v + w] += 0.1              # `Rewarder.goal_bin` (rewarder.py:255-259): the rectangle rows u:u+h, columns v:v+w
  return np.stack([r, g, b], axis=-1)


def rgb_reference(m, n, goal_rect):
  """(rgb0, rgb1) of one env: overhead map m float32 [H, H] with the goal rectangle (u, v, h, w), object map n float32 [h, h]."""
  return _colour(m, goal_rect), _colour(n)


def uint8_reference(m, n, goal_rect):
  """The frames: x * 255 + 0.5 in double, clamped to 0 .. 255, truncated."""
  return tuple(np.clip(x * 255 + 0.5, 0, 255).astype(np.uint8) for x in rgb_reference(m, n, goal_rect))


# ---- wrong variants (tests/test_view.py: each differs from the golden images on at least one case)
def _variant(m, goal_rect, double_division=False, green32=False, no_zero_branch=False, transposed=False):
  m = np.asarray(m, np.float32)
  _max = np.max(m)
  with np.errstate(invalid='ignore', divide='ignore'):
    if double_division:
      r = m.astype(np.float64) / np.float64(_max) if _max != 0 else m.astype(np.float64)
    else:
      r = m / _max if (no_zero_branch or _max != 0) else m
  b = 1 - r
  g = np.ones(r.shape) * 0.5
  if goal_rect is not None:
    u, v, h, w = (int(x) for x in goal_rect)
    if transposed:
      u, v, h, w = v, u, w, h
    if green32:
      g[u:u + h, v:v + w] = np.float32(0.6)
    else:
      g[u:u + h, v:v + w] += 0.1
  return np.stack([r, g, b], axis=-1)


VARIANTS = ('double_division', 'green32', 'no_zero_branch', 'transposed')


def rgb_variant(name, m, n, goal_rect):
  return _variant(m, goal_rect, **{name: True}), _variant(n, None, **{name: True})


def bits_equal(a, b):
  """Same shape, type and bit patterns (so that a NaN equals itself and -0 differs from 0)."""
  a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
  return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- from `VecStackEnv.maps()` to the reference's arguments
def shown_object_map(Om):
  """The object map `render` colours, per env: `maps()` returns [B, h, h], or [B, maps, h, h] with orientation / ordering
  freedom, where map 0 is orientation 0 of the pending rock (of the first rock still unplaced: `n[0]`, env.py:563)."""
  return Om if Om.ndim == 3 else Om[:, 0]


def batch_reference(maps, reference=rgb_reference):
  """`reference` over every env of `maps()` = (Hm, Om, goal), stacked: (rgb0 [B, H, H, 3], rgb1 [B, h, h, 3])."""
  Hm, Om, goal = maps
  Om = shown_object_map(Om)
  out = [reference(Hm[i], Om[i], goal[i]) for i in range(Hm.shape[0])]
  return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
