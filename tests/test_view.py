"""`render('rgb_array')` without a GPU: the numpy restatement the GPU tests compare the kernel with (tests/view_cases.py) equals
the images the reference's own `StackEnv.render` / `TestStackEnv.render` returned (tests/golden/view_golden.npz, made by
tests/golden/make_view_golden.py) bit for bit, the golden cases tell the likely wrong implementations apart from it, and the
export is in the library and in the signature table."""
import ctypes
import os

import numpy as np
import pytest

import view_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def golden():
  g = np.load(os.path.join(HERE, 'golden', 'view_golden.npz'))
  cases = []
  for t in g['cases']:
    n = g[t + '_n']
    cases.append(dict(tag=str(t), m=g[t + '_m'], n=n if n.ndim == 2 else n[0], goal=g[t + '_goal'], rgb0=g[t + '_rgb0'], rgb1=g[t + '_rgb1']))
  return cases


def test_the_golden_cases_cover_the_branches(golden):
  assert len(golden) >= 20
  H = golden[0]['m'].shape[0]
  assert any(c['m'].max() == 0 for c in golden) and any(c['m'].max() > 0 for c in golden)      # env.py:301, both ways
  assert any(c['n'].max() == 0 for c in golden) and any(c['n'].max() > 0 for c in golden)      # env.py:308
  goals = np.array([c['goal'] for c in golden])
  assert (goals[:, 0] == 0).any() and (goals[:, 1] == 0).any() and (goals[:, 1] + goals[:, 3] == H).any()   # goals at the map's edges
  assert any(t['tag'].startswith('v2_') for t in golden)                                        # `TestStackEnv.render`
  for c in golden:
    assert c['m'].dtype == np.float32 and c['n'].dtype == np.float32 and c['rgb0'].dtype == np.float64
    assert c['rgb0'].shape == c['m'].shape + (3,) and c['rgb1'].shape == c['n'].shape + (3,)


def test_the_restatement_equals_the_references_images_bit_for_bit(golden):
  for c in golden:
    rgb0, rgb1 = vc.rgb_reference(c['m'], c['n'], c['goal'])
    assert vc.bits_equal(rgb0, c['rgb0']), c['tag']
    assert vc.bits_equal(rgb1, c['rgb1']), c['tag']


@pytest.mark.parametrize('name', vc.VARIANTS)
def test_the_golden_cases_tell_a_wrong_variant_apart(golden, name):
  differs = 0
  for c in golden:
    rgb0, rgb1 = vc.rgb_variant(name, c['m'], c['n'], c['goal'])
    differs += not (vc.bits_equal(rgb0, c['rgb0']) and vc.bits_equal(rgb1, c['rgb1']))
  assert differs >= 1, name


def test_uint8_frames_round_to_nearest_and_stay_in_range(golden):
  for c in golden:
    f0, f1 = vc.uint8_reference(c['m'], c['n'], c['goal'])
    assert f0.dtype == np.uint8 and f0.shape == c['rgb0'].shape and f1.shape == c['rgb1'].shape
    for f, x in ((f0, c['rgb0']), (f1, c['rgb1'])):
      assert np.abs(f.astype(np.float64) - x * 255).max() <= 0.5
    u, v, h, w = c['goal']
    inside = np.zeros(c['m'].shape, bool)
    inside[u:u + h, v:v + w] = True
    assert (f0[..., 1][inside] == 153).all() and (f0[..., 1][~inside] == 128).all() and (f1[..., 1] == 128).all()


def test_render_rgb_is_exported_and_in_the_signature_table():
  from stackrl_amd import build, lib
  L = ctypes.CDLL(build.build())
  assert hasattr(L, 'srl_render_rgb')
  assert 'srl_render_rgb' in lib.EXPORTS
  res, args = lib._SIGS['srl_render_rgb']
  assert res is ctypes.c_int and list(args) == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def test_render_rgb_refuses_before_it_touches_the_device():
  """A null env and a dtype it does not write: refused in the export's own words, before any HIP call."""
  from stackrl_amd import build, config, lib
  build.build()
  L = lib.load()
  assert L.srl_render_rgb(None, 0, None, None, None) == config.EINVAL
  assert lib.last_error() == 'null env'
