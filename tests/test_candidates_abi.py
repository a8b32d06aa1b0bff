"""CPU tests of the boundary of libstackrl_candidates.so: header <-> `candidates._SIGS` <-> the library's exports, the hash the
library carries, its refusals (each with a text of its own, none of which launches anything), and the packed-fp32 guard of
DESIGN.md section 6a on csrc/candidates.hip and on the shipped library (tests/test_isa_guard.py walks `build.LIBRARIES`; this
library stands in `build.ASSET_LIBRARIES`)."""
import ctypes
import os
import re
import subprocess

import candidates_cases as cases
from stackrl_amd import build, isa_fix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
EXPORTS = ['srl_candidates_build_info', 'srl_candidates_last_error', 'srl_candidates_select']
SOURCE = os.path.join(build.CSRC, 'candidates.hip')
HEADER = os.path.join(ROOT, 'include', 'stackrl_candidates.h')


def _declarations():
  """name -> (return type, [parameter declarations]) of every `ret name(params);` of include/stackrl_candidates.h."""
  with open(HEADER) as f:
    txt = f.read()
  txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
  txt = re.sub(r'^\s*#[^\n]*', '', txt, flags=re.M).replace('extern "C" {', '')
  out = {}
  for ret, name, params in re.findall(r'([A-Za-z_][\w\s\*]*?)\b(srl_\w+)\s*\(([^)]*)\)\s*;', txt):
    assert name not in out
    params = [' '.join(p.split()) for p in params.split(',')]
    out[name] = (' '.join(ret.split()), [] if params == ['void'] else params)
  return out


def _ctype(decl, ret=False):
  if '*' in decl:
    return ctypes.c_char_p if ret and decl.replace(' ', '') == 'constchar*' else ctypes.c_void_p
  base = [t for t in decl.split() if t != 'const'][0]
  return {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int}[base]


def test_header_table_and_exports_agree():
  from stackrl_amd import candidates
  build.build()
  decl = _declarations()
  assert sorted(decl) == EXPORTS and sorted(candidates._SIGS) == EXPORTS
  for name, (ret, params) in decl.items():
    res, args, err = candidates._SIGS[name]
    assert res is _ctype(ret, ret=True), name
    assert list(args) == [_ctype(p) for p in params], name
    assert err == (None if res is ctypes.c_char_p else 'srl_candidates_last_error'), name
  assert decl['srl_candidates_select'][1][-1].replace(' ', '') == 'void*stream'
  # the library exports these and nothing else of the project's; each is defined once, in its one source file
  nm = subprocess.run(['nm', '-D', '--defined-only', build.KLIB], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
  assert sorted(set(re.findall(r'\b(srl_\w+)', nm))) == EXPORTS
  with open(SOURCE) as f:
    defined = re.findall(r'^(?:const char\*|int|int32_t)\s+(srl_\w+)\s*\(', f.read(), re.M)
  assert sorted(defined) == EXPORTS and build.library('candidates').sources == ['candidates.hip']
  # the limits of the header are the binding's and the restatement's
  with open(HEADER) as f:
    limits = dict(re.findall(r'^#define (SRL_CANDIDATES_\w+) (\d+)', f.read(), re.M))
  assert int(limits['SRL_CANDIDATES_MAX_K']) == candidates.MAX_K == cases.MAX_K == 32
  assert int(limits['SRL_CANDIDATES_THREADS']) == cases.THREADS
  # an asset library, and the other libraries are what they were
  assert 'candidates' in build.ASSET_LIBRARIES and 'candidates' not in build.LIBRARIES
  assert build.library('candidates') is build.ASSET_LIBRARIES['candidates']
  assert not any('candidates' in d for name in build.LIBRARIES for d in build.deps(name))
  assert not any('candidates' in d for name in ('rocks', 'valueview') for d in build.deps(name))


def test_library_carries_the_hash_of_its_sources():
  from stackrl_amd import candidates
  build.build()                                   # a no-op unless a library is missing or stale
  i = build.info(build.KLIB)
  assert i is not None and i['variant'] == 'no-slp' and i['hash'] == build.source_hash('candidates')
  assert not build.stale('candidates')
  assert candidates.load().srl_candidates_build_info().decode() == 'SRL_BUILD_INFO<no-slp|{}>'.format(i['hash'])
  assert build.library('candidates').flags is build.QFLAGS
  assert build.deps('candidates') == [os.path.join('include', 'srl_types.h'), os.path.join('include', 'stackrl_candidates.h'),
                                      os.path.join('stackrl_amd', 'csrc', 'candidates.hip')]


def test_the_derived_set_is_the_compilers_and_the_hash_follows_it(tmp_path):
  """What tests/test_build_deps.py holds for the libraries of `build.LIBRARIES`, for this one: `deps` names the project's files
  `hipcc -MM` reads, and the hash moves with each of them and with no file of another library."""
  import shutil
  lib = build.library('candidates')
  keep = [f for f in lib.flags if f not in ('-shared', '-fPIC')]
  mm = subprocess.run([HIPCC] + keep + ['--cuda-host-only', '-MM', '-w', SOURCE], check=True, stdout=subprocess.PIPE,
                      universal_newlines=True).stdout
  files = re.sub(r'\\\n', ' ', mm).split(':', 1)[1].split()
  assert build.deps('candidates') == sorted(os.path.relpath(os.path.realpath(f), os.path.realpath(build.ROOT)) for f in files)
  for d in build.deps('candidates') + build.deps('compare'):
    os.makedirs(os.path.dirname(str(tmp_path / d)), exist_ok=True)
    shutil.copy(os.path.join(build.ROOT, d), str(tmp_path / d))
  root = str(tmp_path)
  assert build.source_hash('candidates', root) == build.source_hash('candidates')
  for d in build.deps('candidates'):
    before = build.source_hash('candidates', root)
    with open(os.path.join(root, d), 'ab') as f:
      f.write(b'\n')
    assert build.source_hash('candidates', root) != before, d
  before = build.source_hash('candidates', root)
  with open(os.path.join(root, 'stackrl_amd', 'csrc', 'compare.hip'), 'ab') as f:
    f.write(b'\n')
  assert build.source_hash('candidates', root) == before


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


def test_no_kernel_of_the_library_contains_the_flagged_packed_form():
  text = build.device_asm(HIPCC, build.QFLAGS, SOURCE)
  assert not isa_fix.flagged(text)
  assert text.count('k_candidates') >= 2 and text.count('s_barrier') >= 4          # the scan saw both kernels
  build.build()
  texts = isa_fix.shipped_asm(build.KLIB)
  assert len(texts) == 1 and not isa_fix.flagged(texts[0])
  assert texts[0].count('k_candidates') >= 2 and texts[0].count('s_barrier') >= 4
