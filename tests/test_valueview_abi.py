"""CPU tests of what only libstackrl_valueview.so has at its boundary: its host-only exports (the layout, the window and the
colour table, held to tests/value_view_cases.py and the matplotlib fixture), its limit, and its refusals (each with a text of
its own, none of which launches anything).  The boundary it shares with the other libraries is held in tests/test_abi.py,
tests/test_build_deps.py and tests/test_isa_guard.py."""
import ctypes
import itertools

import numpy as np

import value_view_cases as cases


def test_the_limit_is_the_comparisons():
  from stackrl_amd import compare, valueview
  assert valueview.MAX_POLICIES == compare.MAX_POLICIES == 8


def test_the_table_is_matplotlibs():
  from stackrl_amd import valueview
  assert np.array_equal(valueview.lut(), cases.golden()['lut'])
  assert valueview.load().srl_valueview_lut(None) == 1 and 'out is null' in valueview.load().srl_valueview_last_error().decode()


def test_layout_and_window_equal_the_restatement():
  from stackrl_amd import valueview
  lib = valueview.load()
  out = (ctypes.c_int32 * 8)()
  for H, h, P, s in itertools.product((1, 8, 16, 33, 128, 1000), (1, 4, 8, 32), range(1, 9), range(1, 9)):
    if h > H:
      continue
    assert lib.srl_valueview_layout(H, h, P, s, out) == 0
    want = cases.layout(H, h, P, s)
    assert list(out) == [want[k] for k in ('FH', 'FW', 'nv', 'ncol', 'nline', 'TB')] + [cases.window(P, 0), cases.window(P, P - 1)]
    assert valueview.layout(H, h, P, s) == {k: want[k] for k in ('FH', 'FW', 'nv', 'ncol', 'nline', 'TB')}
  assert (valueview.layout(128, 32, 6, 1)['FH'], valueview.layout(128, 32, 6, 1)['FW']) == (230, 477)
  for P in range(1, 9):
    for index in range(P):
      assert valueview.window(P, index) == cases.window(P, index)
    assert valueview.tile_order(['p{}'.format(j) for j in range(P)], P - 1) == ['p{}'.format(j) for j in range(max(0, P - 6), P)]
  for bad in ((8, 9, 1, 1), (8, 0, 1, 1), (8, 4, 0, 1), (8, 4, 9, 1), (8, 4, 1, 0), (8, 4, 1, 9), (30000, 1, 3, 8)):
    assert lib.srl_valueview_layout(*bad, out) == 1 and 'no frame for' in lib.srl_valueview_last_error().decode()
  assert lib.srl_valueview_layout(8, 4, 1, 1, None) == 1
  m = ctypes.c_int32()
  assert lib.srl_valueview_window(9, 0, ctypes.byref(m)) == 1 and 'got 9' in lib.srl_valueview_last_error().decode()
  assert lib.srl_valueview_window(3, 3, ctypes.byref(m)) == 1 and 'index must be in 0..2, got 3' in lib.srl_valueview_last_error().decode()
  assert lib.srl_valueview_window(3, 0, None) == 1


def test_each_refusal_has_its_own_text_and_launches_nothing():
  """The refusals return before any HIP call, so they can be taken on a machine without a device: the pointers are never
  dereferenced (1 stands for a non-null device pointer)."""
  from stackrl_amd import valueview
  lib = valueview.load()

  def refused(P=2, maps=(1,) * 8, mask=0, B=2, G=1, H=16, h=8, rgb0=1, rgb1=1, actions=None, indexes=1, n=2, index=0, scale=2,
              mark=0, scratch=1, frames=4):
    rc = lib.srl_valueview_frames(P, *maps, mask, B, G, H, h, rgb0, rgb1, actions, indexes, n, index, scale, mark, scratch, frames, None)
    assert rc == 1
    return lib.srl_valueview_last_error().decode()

  texts = {
    'P0': refused(P=0), 'P9': refused(P=9), 'index-1': refused(index=-1), 'index2': refused(index=2), 'scale0': refused(scale=0),
    'scale9': refused(scale=9), 'n0': refused(n=0), 'B0': refused(B=0), 'G0': refused(G=0), 'h0': refused(h=0),
    'H<h': refused(H=7, h=8), 'GA': refused(G=2, H=32768, h=1), 'A': refused(H=60000, h=1),
    'map1': refused(maps=(1, None, 1, 1, 1, 1, 1, 1)), 'rgb0': refused(rgb0=None), 'rgb1': refused(rgb1=None),
    'indexes': refused(indexes=None), 'scratch': refused(scratch=None), 'frames': refused(frames=None),
    'size': refused(H=4096, h=4096, n=40, scale=8), 'align': refused(frames=6),
  }
  assert 'frames must be 4-byte aligned' in texts['align']
  assert 'the number of policies must be in 1..8, got 0' in texts['P0'] and 'got 9' in texts['P9']
  assert 'index must be in 0..1, got -1' in texts['index-1'] and 'got 2' in texts['index2']
  assert 'scale must be in 1..8, got 0' in texts['scale0'] and 'got 9' in texts['scale9']
  assert 'n must be at least 1, got 0' in texts['n0']
  assert 'B must be at least 1, got 0' in texts['B0']
  assert 'G must be at least 1, got 0' in texts['G0']
  assert 'got H 16, h 0' in texts['h0'] and 'got H 7, h 8' in texts['H<h']
  assert 'G * A must be at most 2^31-2, got 2 * 1073741824' in texts['GA'] and 'got 1 * 3600000000' in texts['A']
  assert 'map 1 of 2 policies is null' in texts['map1']
  for key, word in (('rgb0', 'rgb0 0'), ('rgb1', 'rgb1 0'), ('indexes', 'indexes 0'), ('scratch', 'range_scratch 0'), ('frames', 'frames 0')):
    assert 'a required pointer is null' in texts[key] and word in texts[key]
  assert 'the frames must fit 2^31-1 bytes, got n 40' in texts['size']
  # a null map beyond P is not looked at, nor are null actions: the next refusal is reached
  assert 'frames 0' in refused(P=1, maps=(1,) + (None,) * 7, frames=None)
  assert len(set(texts.values())) == len(texts)
  assert len({t.split(',')[0] for t in texts.values()}) >= 12
