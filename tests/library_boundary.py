"""The boundary of the native libraries, stated once: the readers the boundary tests share (a header's declarations, their
ctypes types, a library's exports, where its sources define them, what the compiler reads for it) and `ROWS`, one row per
library of `build.LIBRARIES` with what really differs between them.  tests/test_abi.py, tests/test_build_deps.py and
tests/test_isa_guard.py run their assertions over `sorted(build.LIBRARIES)`; a new library brings a row here and a census
in `test_isa_guard._SAW`."""
import collections
import ctypes
import importlib
import os
import re
import subprocess

from stackrl_amd import build

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
TYPES = os.path.join('include', 'srl_types.h')      # the one file two libraries' dependency sets may share
_CTYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
           'float': ctypes.c_float, 'double': ctypes.c_double}


def header_text(header):
  """include/`header` without its comments (both kinds), preprocessor lines and `extern "C" {`."""
  with open(os.path.join(build.ROOT, 'include', header)) as f:
    txt = f.read()
  txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
  txt = re.sub(r'//[^\n]*', '', txt)
  return re.sub(r'^\s*#[^\n]*', '', txt, flags=re.M).replace('extern "C" {', '')


def declarations(headers):
  """name -> (return type, [parameter declarations]) of every `ret srl_name(params);` of the headers, `typedef struct` bodies
  left out; a name declared twice fails here."""
  out = {}
  for h in headers:
    txt = re.sub(r'typedef struct\s+\w*\s*\{.*?\}\s*\w+;', '', header_text(h), flags=re.S)
    for ret, name, params in re.findall(r'([A-Za-z_][\w\s\*]*?)\b(srl_\w+)\s*\(([^)]*)\)\s*;', txt):
      assert name not in out, name + ' is declared twice'
      params = [' '.join(p.split()) for p in params.split(',')]
      out[name] = (' '.join(ret.split()), [] if params == ['void'] else params)
  return out


def ctype(decl, ret=False):
  """The ctypes type of a return type or a parameter declaration: any pointer is void*, but a returned const char* a string."""
  if '*' in decl:
    return ctypes.c_char_p if ret and decl.replace(' ', '') == 'constchar*' else ctypes.c_void_p
  return _CTYPES[[t for t in decl.split() if t != 'const'][0]]


def exports(name):
  """The `srl_` names among the dynamic symbols the built library defines."""
  nm = subprocess.run(['nm', '-D', '--defined-only', build.LIBRARIES[name].path], check=True, stdout=subprocess.PIPE,
                      universal_newlines=True).stdout
  return sorted(set(re.findall(r'\b(srl_\w+)', nm)))


def defined(name):
  """export -> (source file, return type) of every `srl_` function the library's sources define at the start of a line; a name
  defined twice fails here."""
  out = {}
  for s in build.LIBRARIES[name].sources:
    with open(os.path.join(build.CSRC, s)) as f:
      for ret, export in re.findall(r'^(const char\*|void|int|int32_t|int64_t)\s+(srl_\w+)\s*\(', f.read(), re.M):
        assert export not in out, export + ' is defined twice'
        out[export] = (s, ret)
  return out


def compiler_deps(name):
  """The project's files that the compiler reads for the library's sources with the library's flags (`hipcc -MM`), relative
  to the repository, plus the recipe files."""
  lib = build.LIBRARIES[name]
  keep = [f for f in lib.flags if f not in ('-shared', '-fPIC')]
  out = set(lib.recipe)
  for s in lib.sources:
    mm = subprocess.run([HIPCC] + keep + ['--cuda-host-only', '-MM', '-w', os.path.join(build.CSRC, s)], check=True,
                        stdout=subprocess.PIPE, universal_newlines=True).stdout
    files = re.sub(r'\\\n', ' ', mm).split(':', 1)[1].split()
    out.update(os.path.relpath(os.path.realpath(f), os.path.realpath(build.ROOT)) for f in files)
  assert not any(d.startswith('..') for d in out), out         # -MM leaves system headers out
  return sorted(out)


# headers:     the headers that declare the library's exports
# module:      the wrapper that holds its `_SIGS` and `load`
# build_info:  its `*_build_info` export
# names:       the exports by name, where the per-library test listed them (None: the count is held where it was, test_abi.py)
# untyped:     None, or why only the names of `_SIGS` are held to the header and not the types
# extra:       None, or why the library exports and defines more `srl_` names than its header declares
# host_only:   exports that return a status (`int`) and launch nothing: every other one that returns `int` takes the stream last
# accessor:    (export, declared return type) -> the error accessor `_SIGS` must name for it; None: no shared rule applies
# deps:        the literal dependency set (the single-source libraries), or None: held to the compiler alone (test_build_deps.py)
Row = collections.namedtuple('Row', 'headers module build_info names untyped extra host_only accessor deps')


def _single(name, names, host_only, accessor, deps):
  """The row of a library of one source, one header and one accessor."""
  return Row(('stackrl_{}.h'.format(name),), name, 'srl_{}_build_info'.format(name), names, None, None, host_only, accessor,
             [os.path.normpath(d) for d in deps.split()])


ROWS = {
  'env': Row(('stackrl_hip.h',), 'lib', 'srl_build_info', None,
             'its table passes POINTER(CConfig) and POINTER(c_void_p) where the header says srl_config* and srl_env**',
             'the kernels (srl_k_*) are dynamic symbols too, and stackrl_hip.hip defines srl_debug_* for diagnostic builds only',
             (), None, None),      # the handle API reports its errors per call (env.py `_check`): `_SIGS` names no accessor
  'qnet': Row(('stackrl_qnet.h', 'stackrl_explore.h', 'stackrl_greedy.h', 'stackrl_baseline_rows.h'), 'qops',
              'srl_qnet_build_info', None, None, None, (),
              None, None),         # an accessor per source file: test_abi.py test_qnet_error_accessors_match_the_sources
  'compare': _single('compare', ['srl_compare_build_info', 'srl_compare_last_error', 'srl_compare_record_doubles', 'srl_compare_step'],
                     (), lambda export, ret: 'srl_compare_last_error' if ret == 'int' else None,
                     'include/stackrl_compare.h stackrl_amd/csrc/compare.hip'),
  'rocks': _single('rocks', ['srl_rocks_build_info', 'srl_rocks_generate', 'srl_rocks_last_error', 'srl_rocks_points'],
                   ('srl_rocks_points',), lambda export, ret: 'srl_rocks_last_error' if export == 'srl_rocks_generate' else None,
                   'include/srl_types.h include/stackrl_rocks.h stackrl_amd/csrc/rocks.hip'),
  'valueview': _single('valueview', ['srl_valueview_build_info', 'srl_valueview_frames', 'srl_valueview_last_error',
                                     'srl_valueview_layout', 'srl_valueview_lut', 'srl_valueview_window'],
                       ('srl_valueview_layout', 'srl_valueview_lut', 'srl_valueview_window'),
                       lambda export, ret: None if ret == 'const char*' else 'srl_valueview_last_error',
                       'include/srl_types.h include/stackrl_valueview.h stackrl_amd/csrc/valueview.hip'),
  'candidates': _single('candidates', ['srl_candidates_build_info', 'srl_candidates_last_error', 'srl_candidates_select'],
                        (), lambda export, ret: None if ret == 'const char*' else 'srl_candidates_last_error',
                        'include/srl_types.h include/stackrl_candidates.h stackrl_amd/csrc/candidates.hip'),
}


def module(name):
  return importlib.import_module('stackrl_amd.' + ROWS[name].module)
