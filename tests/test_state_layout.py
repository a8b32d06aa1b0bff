"""CPU tests of the state-record exports (include/stackrl_hip.h "State records"): the layout query against its restatement
(tests/state_cases.py), and the refusals that come before any HIP call."""
import ctypes
import itertools

import pytest

import state_cases as sc

_P = 64      # a non-null pointer: a refusal comes before anything is read through it


@pytest.fixture(scope='module')
def L():
  from stackrl_amd import lib
  return lib.load()


def _layout(L, **kw):
  from stackrl_amd.config import StackConfig
  c = StackConfig(**kw).to_c()
  words = ctypes.c_int64()
  off = (ctypes.c_int64 * 4)()
  assert L.srl_state_layout(ctypes.byref(c), ctypes.byref(words), off) == 0
  return int(words.value), [int(o) for o in off]


def test_word_constants_are_read_from_the_sources():
  assert sc.D['SRL_GM_WORDS'] == 1 + 5 * sc.D['SRL_GMAXP'] and sc.D['SRL_MAN_WORDS'] > 0
  assert sc.D['SRL_STAGE_STRIDE'] == sc.D['SRL_STAGE_HDR'] + sc.D['SRL_MAX_TRIS'] + 2


def test_layout_export_matches_the_restated_record(L):
  stride = int(L.srl_stage_record_stride())
  assert stride == sc.D['SRL_STAGE_STRIDE']
  seen = {}
  for ep, rf, osr in itertools.product(range(1, 33), (3, 4, 5), (3, 4)):
    want = sc.expected(ep, rf, osr, stride)
    for of, order in ((0, False), (2, True)):
      got = _layout(L, episode_length=ep, resolution_factor=rf, observable_size_ratio=osr, orientation_freedom=of, ordering_freedom=order)
      assert got == want, (ep, rf, osr, of, order)
      assert all(o % 4 == 0 for o in got[1]) and got[0] % 4 == 0 and got[1][0] == 0
    seen[(ep, rf, osr)] = want[0]
  # the record size changes exactly when one of the inputs changes: no two of the 192 shapes share a size (and the
  # freedoms, compared above, do not enter)
  assert len(set(seen.values())) == len(seen) == 32 * 3 * 2


def test_layout_python_wrapper_and_the_query_needs_no_handle(L):
  from stackrl_amd import state
  from stackrl_amd.config import StackConfig
  words, off = state.layout(StackConfig(episode_length=8, n_envs=1024))
  assert (words, [off[p] for p in state.PARTS]) == sc.expected(8, 5, 4, int(L.srl_stage_record_stride()))
  assert words * 4 > 100000          # about 100 KB per env at 8 rocks and 128 x 128 maps
  assert state.layout(StackConfig(episode_length=8, n_envs=3, env_index_offset=7))[0] == words
  with pytest.raises(ValueError):
    bad = StackConfig(episode_length=8)
    bad.observable_size_ratio = 9       # 288 x 288: srl_create refuses it, and so does the query, in the same words
    state.layout(bad)


# (export, arguments, the text left in srl_last_error): every refusal below comes before any HIP call and needs no handle
_REFUSED = [
  ('srl_state_layout', (None, None, None), 'srl_state_layout: null config'),
  ('srl_state_signature', (None, None), 'srl_state_signature: null output'),
  ('srl_state_signature', (None, _P), 'srl_state_signature: null env'),
  # env, idx, n, records, &seed, &sample_counter, stream
  ('srl_state_get', (None, None, 1, None, None, None, None), 'srl_state_get: null records buffer'),
  ('srl_state_get', (None, None, 0, _P, None, None, None), 'srl_state_get: n must be at least 1'),
  ('srl_state_get', (None, _P, -3, _P, None, None, None), 'srl_state_get: n must be at least 1'),
  ('srl_state_get', (None, None, 1, _P, None, None, None), 'srl_state_get: null env'),
  # env, signature, dst, src, n, records, stream
  ('srl_state_set', (None, 1, None, None, 1, None, None), 'srl_state_set: null records buffer'),
  ('srl_state_set', (None, 1, None, None, 0, _P, None), 'srl_state_set: n must be at least 1'),
  ('srl_state_set', (None, 1, _P, _P, 1, _P, None), 'srl_state_set: null env'),
  ('srl_state_set_rng', (None, 1, 2), 'srl_state_set_rng: null env'),
]


def test_state_exports_refuse_bad_arguments_with_their_own_text(L):
  """Null handle, null buffer and n < 1, each with its own text, before any HIP call (there is no device here).  The
  refusal of a foreign signature needs a handle to compare with: tests/test_state_gpu.py."""
  from stackrl_amd import config, lib
  assert {n for n, _, _ in _REFUSED} == {n for n in lib.EXPORTS if n.startswith('srl_state_')} and len(_REFUSED) == 11
  for name, args, text in _REFUSED:
    assert getattr(L, name)(*args) == config.EINVAL, (name, args)
    assert lib.last_error() == text, (name, args)
