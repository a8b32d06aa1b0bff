"""CPU tests of what only libstackrl_candidates.so has at its boundary: the limits of its header, and its refusals (each with
a text of its own, none of which launches anything).  The boundary it shares with the other libraries is held in
tests/test_abi.py, tests/test_build_deps.py and tests/test_isa_guard.py."""
import os
import re

import candidates_cases as cases
from stackrl_amd import build


def test_the_limits_of_the_header_are_the_bindings_and_the_restatements():
  from stackrl_amd import candidates
  with open(os.path.join(build.ROOT, 'include', 'stackrl_candidates.h')) as f:
    limits = dict(re.findall(r'^#define (SRL_CANDIDATES_\w+) (\d+)', f.read(), re.M))
  assert int(limits['SRL_CANDIDATES_MAX_K']) == candidates.MAX_K == cases.MAX_K == 32
  assert int(limits['SRL_CANDIDATES_THREADS']) == cases.THREADS


def test_each_refusal_has_its_own_text_and_launches_nothing():
  """The refusals return before any HIP call, so they can be taken on a machine without a device: the pointers are never
  dereferenced (8 stands for a non-null device pointer)."""
  from stackrl_amd import candidates
  lib = candidates.load()

  def refused(values=8, f64=0, action=None, B=2, G=2, OH=5, n_valid=2, k=4, radius=1, cand=8, count=8):
    rc = lib.srl_candidates_select(values, f64, action, B, G, OH, n_valid, k, radius, cand, count, None)
    assert rc == 1
    return lib.srl_candidates_last_error().decode()

  texts = {
    'B0': refused(B=0), 'B-1': refused(B=-1), 'G0': refused(G=0), 'OH0': refused(OH=0), 'GA': refused(G=2, OH=32768),
    'A': refused(G=1, OH=60000), 'n_valid0': refused(n_valid=0), 'n_valid3': refused(n_valid=3), 'k0': refused(k=0),
    'k33': refused(k=33), 'radius': refused(radius=-1), 'values': refused(values=None),
    'cand': refused(cand=None), 'count': refused(count=None),
  }
  assert 'B must be at least 1, got 0' in texts['B0'] and 'got -1' in texts['B-1']
  assert 'G must be at least 1, got 0' in texts['G0']
  assert 'OH must be at least 1, got 0' in texts['OH0']
  assert 'G * A must be at most 2^31-2, got 2 * 1073741824' in texts['GA'] and 'got 1 * 3600000000' in texts['A']
  assert 'n_valid must be in 1..2, got 0' in texts['n_valid0'] and 'got 3' in texts['n_valid3']
  assert 'k must be in 1..32, got 0' in texts['k0'] and 'got 33' in texts['k33']
  assert 'radius must be at least 0, got -1' in texts['radius']
  for key, word in (('values', 'values 0'), ('cand', 'cand 0'), ('count', 'count 0')):
    assert 'a required pointer is null' in texts[key] and word in texts[key]
  assert all(t.startswith('srl_candidates_select: ') for t in texts.values())
  assert len(set(texts.values())) == len(texts)
  assert len({t.split(',')[0] for t in texts.values()}) >= 9
  # null actions are an input of their own, not a refusal, and both element types pass the checks: the next refusal is reached
  assert 'count 0' in refused(action=None, f64=1, count=None) and 'count 0' in refused(action=8, count=None)
  # a k beyond the entries considered is exhaustion, not a refusal
  assert 'cand 0' in refused(G=3, OH=2, n_valid=1, k=5, cand=None)
  # the largest k, radius and map the checks admit are not refused for their size: the null output is
  assert 'cand 0' in refused(G=1, OH=46340, n_valid=1, k=32, radius=2 ** 31 - 1, cand=None)
