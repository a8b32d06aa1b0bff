"""CPU tests of the definition of include/stackrl_valueview.h as tests/value_view_cases.py restates it: the restatement gives
matplotlib's bytes on every committed map (and on a fresh `to_rgba` where matplotlib imports), every named wrong variant is told
from it by a committed case, and the window and layout closed forms hold."""
import itertools

import numpy as np
import pytest

import value_view_cases as cases


def _maps():
  g = cases.golden()
  return list(zip([str(n) for n in g['names']], g['maps'], g['rgba']))


def test_the_fixture_holds_the_cases_the_definition_turns_on():
  names = [n for n, _, _ in _maps()]
  g = cases.golden()
  assert g['lut'].shape == (256, 3) and g['lut'].dtype == np.uint8 and g['maps'].dtype == np.float32
  assert tuple(g['lut'][255]) == (253, 231, 36) and tuple(g['lut'][0]) == (68, 1, 84)
  for want in ('random 1e-6', 'random 1e4', 'constant', 'nan and infinities', 'non-finite at the extremes', 'all non-finite',
               'tied maxima', 'bin edges vmin 0.0 span 0.1', 'bin edges vmin 0.0 span 3.0', 'bin edges vmin 0.0 span 7.0',
               'bin edges vmin 2.5 span 3.0'):
    assert want in names
  by = dict((n, v) for n, v, _ in _maps())
  assert not np.isfinite(by['all non-finite']).any()
  v = by['non-finite at the extremes']
  assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
  v = by['tied maxima']
  assert np.count_nonzero(v == v.max()) > 1
  assert len(set(by['constant'].ravel())) == 1


@pytest.mark.parametrize('name,v,rgba', _maps(), ids=[n for n, _, _ in _maps()])
def test_restatement_equals_the_golden_image(name, v, rgba):
  got = cases.colour_cells(v)
  fin = np.isfinite(v)
  assert np.array_equal(got[fin], rgba[..., :3][fin])
  assert np.all(rgba[..., 3][fin] == 255) and np.all(rgba[..., 3][~fin] == 0)      # matplotlib masks what is not finite
  assert np.all(got[~fin] == cases.BACKGROUND)


def test_restatement_equals_a_fresh_to_rgba():
  matplotlib = pytest.importorskip('matplotlib')
  matplotlib.use('Agg')
  import matplotlib.pyplot as plt
  from matplotlib import cm
  assert np.array_equal((np.array(cm.viridis.colors) * 255).astype(np.uint8), cases.golden()['lut'])
  rng = np.random.RandomState(5)
  _, ax = plt.subplots()
  maps = [v for _, v, _ in _maps() if np.isfinite(v).any()]
  for e in (-4, -1, 0, 2, 6):
    maps += [(rng.standard_normal((7, 5)) * 10.0 ** e + rng.uniform(-3, 3)).astype(np.float32) for _ in range(8)]
  for v in maps:
    ax.cla()
    im = ax.imshow(v)
    want = im.to_rgba(im.get_array(), bytes=True)
    fin = np.isfinite(v)
    assert np.array_equal(cases.colour_cells(v)[fin], want[..., :3][fin])
    assert np.all(want[..., 3][~fin] == 0)
  plt.close('all')


@pytest.mark.parametrize('variant', cases.CELL_VARIANTS)
def test_each_cell_variant_differs_on_a_committed_map(variant):
  differing = [n for n, v, rgba in _maps()
               if not np.array_equal(cases.colour_cells(v, variant)[np.isfinite(v)], rgba[..., :3][np.isfinite(v)])]
  assert differing, cases.VARIANTS[variant]
  if variant == 'float64':
    assert 'bin edges vmin 0.0 span 0.1' in differing
  if variant == 'all_cells':
    assert 'nan and infinities' in differing


def _frame_inputs():
  return cases.synthetic(B=2, H=8, h=4, P=8, G=1, seed=3)


def test_window_and_ring_variants_differ_on_frames():
  rgb0, rgb1, values, actions = _frame_inputs()
  for variant, index in (('window_noclip', 0), ('window_noclip', 7), ('ring_tile_index', 5), ('ring_tile_index', 7)):
    right = cases.reference_frames(rgb0, rgb1, values, actions, index=index, scale=1)
    wrong = cases.reference_frames(rgb0, rgb1, values, actions, index=index, scale=1, variant=variant)
    assert right.shape == wrong.shape and not np.array_equal(right, wrong), (variant, index)
  # where clip and window agree, so do the frames
  right = cases.reference_frames(rgb0, rgb1, values, actions, index=4, scale=1)
  assert np.array_equal(right, cases.reference_frames(rgb0, rgb1, values, actions, index=4, scale=1, variant='window_noclip'))
  for variant in cases.CELL_VARIANTS:
    assert variant in cases.VARIANTS
  assert set(cases.VARIANTS) == set(cases.CELL_VARIANTS) | {'window_noclip', 'ring_tile_index'}


def test_window_is_the_clipped_centre():
  for P in range(1, 9):
    nv = min(P, 6)
    for index in range(P):
      w = cases.window(P, index)
      assert w == np.clip(index - nv // 2, 0, P - nv)
      assert 0 <= w <= index < w + nv <= P                       # the driving policy is always shown


def test_layout_closed_forms():
  l = cases.layout(128, 32, 6, 1)
  assert (l['FH'], l['FW']) == (230, 477)
  for H, h, P, s in itertools.product((1, 8, 16, 33, 128), (1, 4, 8, 32), range(1, 9), (1, 2, 3, 8)):
    if h > H:
      continue
    l = cases.layout(H, h, P, s)
    reg = cases.regions(H, h, P, s)
    assert len(reg) == 2 + min(P, 6)
    boxes = list(reg.values())
    for r0, r1, c0, c1 in boxes:
      assert 0 <= r0 < r1 <= l['FH'] - cases.GAP + cases.GAP and 0 <= c0 < c1 <= l['FW']
      assert r1 <= l['FH'] and r0 >= cases.GAP and c0 >= cases.GAP
    for (a0, a1, b0, b1), (c0, c1, d0, d1) in itertools.combinations(boxes, 2):
      assert a1 <= c0 or c1 <= a0 or b1 <= d0 or d1 <= b0
    assert l['FW'] == max(c1 for _, _, _, c1 in boxes) + cases.GAP
    assert l['FH'] == max(r1 for _, r1, _, _ in boxes) + cases.GAP


def test_frames_place_views_tiles_ring_and_marks():
  rgb0, rgb1, values, actions = cases.synthetic(B=3, H=8, h=4, P=3, G=2, seed=1, corners=True)
  s, index = 2, 1
  frames = cases.reference_frames(rgb0, rgb1, values, actions, index=index, indexes=[2, 0], scale=s, mark=True)
  plain = cases.reference_frames(rgb0, rgb1, values, actions, index=index, indexes=[2, 0], scale=s, mark=False)
  reg = cases.regions(8, 4, 3, s)
  l = cases.layout(8, 4, 3, s)
  assert frames.shape == (2, l['FH'], l['FW'], 3)
  r0, r1, c0, c1 = reg['overhead']
  assert np.array_equal(plain[0, r0:r1:s, c0:c1:s], rgb0[2]) and np.array_equal(plain[1, r0 + 1:r1:s, c0 + 1:c1:s], rgb0[0])
  r0, r1, c0, c1 = reg['object']
  assert np.array_equal(plain[0, r0:r1:s, c0:c1:s], rgb1[2])
  ring = cases.golden()['lut'][255]
  for k in range(3):
    r0, r1, c0, c1 = reg['tile{}'.format(k)]
    assert np.all(plain[0, r0, c0:c1] == (ring if k == index else cases.BACKGROUND))
    A = 25
    a = int(actions[k][2])
    x = values[k].reshape(3, 2, A)[2, a // A]
    inner = plain[0, r0 + 3:r1 - 3:s, c0 + 3:c1 - 3:s]
    assert np.array_equal(inner, cases.colour_cells(x).reshape(5, 5, 3))
    u, v = divmod(a % A, 5)
    marked = frames[0, r0 + 3:r1 - 3:s, c0 + 3:c1 - 3:s]
    assert tuple(marked[u, v]) == (255, 0, 0) and np.count_nonzero((marked != inner).any(-1)) <= 1
  outside = np.ones(frames.shape[1:3], bool)
  for r0, r1, c0, c1 in reg.values():
    outside[r0:r1, c0:c1] = False
  assert np.all(frames[:, outside] == 255)
  # the marks of the overhead view: the outline of the driving policy's window, and nothing else changes there
  r0, r1, c0, c1 = reg['overhead']
  u, v = divmod(int(actions[index][2]) % 25, 5)
  changed = (frames[0, r0:r1:s, c0:c1:s] != plain[0, r0:r1:s, c0:c1:s]).any(-1)
  want = np.zeros((8, 8), bool)
  want[u:u + 4, v:v + 4] = True
  want[u + 1:u + 3, v + 1:v + 3] = False
  assert not np.any(changed & ~want)
  assert np.all(frames[0, r0:r1:s, c0:c1:s][want] == cases.RED)
