"""CPU tests of the boundary of libstackrl_compare.so: header <-> `compare._SIGS` <-> the library's exports, the hash the
library carries, and the packed-fp32 guard of DESIGN.md section 6a on csrc/compare.hip and on the shipped library (as
tests/test_isa_guard.py applies it to the other two)."""
import ctypes
import os
import re
import subprocess

from stackrl_amd import build, isa_fix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def _declarations():
  """name -> (return type, [parameter declarations]) of every `ret name(params);` of include/stackrl_compare.h."""
  with open(os.path.join(ROOT, 'include', 'stackrl_compare.h')) as f:
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
  from stackrl_amd import compare
  build.build()
  decl = _declarations()
  assert sorted(decl) == ['srl_compare_build_info', 'srl_compare_last_error', 'srl_compare_record_doubles', 'srl_compare_step']
  assert sorted(compare._SIGS) == sorted(decl)
  for name, (ret, params) in decl.items():
    res, args, err = compare._SIGS[name]
    assert res is _ctype(ret, ret=True), name
    assert list(args) == [_ctype(p) for p in params], name
    if ret == 'int':                   # the launching export: the stream goes last, its refusals are read through the accessor
      assert params[-1].replace(' ', '') == 'void*stream' and err == 'srl_compare_last_error'
    else:
      assert err is None
  # the library exports these and nothing else of the project's
  nm = subprocess.run(['nm', '-D', '--defined-only', build.CLIB], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
  assert sorted(set(re.findall(r'\b(srl_\w+)', nm))) == sorted(decl)
  # defined once, in the library's one source file
  with open(os.path.join(build.CSRC, 'compare.hip')) as f:
    defined = re.findall(r'^(?:const char\*|int|int32_t)\s+(srl_\w+)\s*\(', f.read(), re.M)
  assert sorted(defined) == sorted(decl) and build.LIBRARIES['compare'].sources == ['compare.hip']
  lib = compare.load()
  for P in range(0, 10):
    assert lib.srl_compare_record_doubles(P) == (compare.record_doubles(P) if 1 <= P <= 8 else 0)
  assert compare.record_doubles(8) == 189 and compare.MAX_POLICIES == 8
  # the other libraries are what they were
  assert 'compare.hip' not in build.QSRC and not any('compare' in d for d in build.deps('qnet'))


def test_library_carries_the_hash_of_its_sources():
  from stackrl_amd import compare
  build.build()                                   # a no-op unless a library is missing or stale
  i = build.info(build.CLIB)
  assert i is not None and i['variant'] == 'no-slp' and i['hash'] == build.source_hash('compare')
  assert not build.stale('compare')
  assert compare.load().srl_compare_build_info().decode() == 'SRL_BUILD_INFO<no-slp|{}>'.format(i['hash'])
  assert '-fno-slp-vectorize' in build.LIBRARIES['compare'].flags
  # the hash follows the header and the source: the set derived from the source's includes is exactly these two
  assert build.deps('compare') == [os.path.join('include', 'stackrl_compare.h'), os.path.join('stackrl_amd', 'csrc', 'compare.hip')]


def test_no_kernel_of_the_library_contains_the_flagged_packed_form():
  text = build.device_asm(HIPCC, build.QFLAGS, os.path.join(build.CSRC, 'compare.hip'))
  assert not isa_fix.flagged(text)
  assert text.count('k_compare') >= 8 and 'k_fold' in text and 'v_fma_f64' in text       # the scan saw the kernels
  build.build()
  texts = isa_fix.shipped_asm(build.CLIB)
  assert len(texts) == 1
  assert not isa_fix.flagged(texts[0])
  assert texts[0].count('k_compare') >= 8 and 'v_fma_f64' in texts[0]
  assert 'scratch_' not in texts[0]                # nothing spills to memory (P = 8: 36 float64 sums and 72 counts a thread)
