"""CPU tests of the boundary of libstackrl_rocks.so: header <-> `rocks._SIGS` / `rocks.Params` <-> the library's exports, the
hash the library carries, its refusals (each with a text of its own, none of which launches anything), and the packed-fp32 guard of DESIGN.md section 6a on csrc/rocks.hip and on the shipped library
(tests/test_isa_guard.py walks `build.LIBRARIES`; this library stands in `build.ASSET_LIBRARIES`)."""
import ctypes
import os
import re
import subprocess

from stackrl_amd import build, isa_fix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
EXPORTS = ['srl_rocks_build_info', 'srl_rocks_generate', 'srl_rocks_last_error', 'srl_rocks_points']


def _header():
  with open(os.path.join(ROOT, 'include', 'stackrl_rocks.h')) as f:
    txt = f.read()
  txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
  return re.sub(r'^\s*#[^\n]*', '', txt, flags=re.M).replace('extern "C" {', '')


def _declarations():
  """name -> (return type, [parameter declarations]) of every `ret name(params);` of include/stackrl_rocks.h."""
  txt = re.sub(r'typedef struct.*?\}\s*\w+;', '', _header(), flags=re.S)
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
  return {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'uint32_t': ctypes.c_uint32,
          'float': ctypes.c_float}[base]


def test_header_table_struct_and_exports_agree():
  from stackrl_amd import rocks
  build.build()
  decl = _declarations()
  assert sorted(decl) == EXPORTS and sorted(rocks._SIGS) == EXPORTS
  for name, (ret, params) in decl.items():
    res, args, err = rocks._SIGS[name]
    assert res is _ctype(ret, ret=True), name
    assert list(args) == [_ctype(p) for p in params], name
  assert decl['srl_rocks_generate'][1][-1].replace(' ', '') == 'void*stream'
  assert rocks._SIGS['srl_rocks_generate'][2] == 'srl_rocks_last_error'
  # the parameter struct, field by field
  body = re.search(r'typedef struct srl_rocks_params \{(.*?)\}\s*srl_rocks_params;', _header(), re.S).group(1)
  fields = []
  for typ, names in re.findall(r'(\w+)\s+([^;]+);', body):
    for n in names.split(','):
      m = re.match(r'\s*(\w+)(?:\[(\d+)\])?\s*$', n)
      fields.append((m.group(1), _ctype(typ) * int(m.group(2)) if m.group(2) else _ctype(typ)))
  assert [(n, t) for n, t in rocks.Params._fields_] == fields and ctypes.sizeof(rocks.Params) == 40
  # the library exports these and nothing else of the project's; they are defined once, in its one source file
  nm = subprocess.run(['nm', '-D', '--defined-only', build.RLIB], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
  assert sorted(set(re.findall(r'\b(srl_\w+)', nm))) == EXPORTS
  with open(os.path.join(build.CSRC, 'rocks.hip')) as f:
    defined = re.findall(r'^(?:const char\*|int|int32_t)\s+(srl_\w+)\s*\(', f.read(), re.M)
  assert sorted(defined) == EXPORTS and build.library('rocks').sources == ['rocks.hip']
  # the limits are the env's, and the other libraries are what they were
  assert (rocks.MAX_VERTS, rocks.MAX_TRIS, rocks.MAX_POINTS) == (128, 252, 386)
  assert 'rocks' in build.ASSET_LIBRARIES and 'rocks' not in build.LIBRARIES and build.library('rocks') is build.ASSET_LIBRARIES['rocks']
  assert not any('rocks' in d for name in build.LIBRARIES for d in build.deps(name))


def test_library_carries_the_hash_of_its_sources():
  from stackrl_amd import rocks
  build.build()                                   # a no-op unless a library is missing or stale
  i = build.info(build.RLIB)
  assert i is not None and i['variant'] == 'no-slp' and i['hash'] == build.source_hash('rocks')
  assert not build.stale('rocks')
  assert rocks.load().srl_rocks_build_info().decode() == 'SRL_BUILD_INFO<no-slp|{}>'.format(i['hash'])
  assert build.library('rocks').flags is build.QFLAGS
  assert build.deps('rocks') == [os.path.join('include', 'srl_types.h'), os.path.join('include', 'stackrl_rocks.h'),
                                 os.path.join('stackrl_amd', 'csrc', 'rocks.hip')]


def test_the_derived_set_is_the_compilers_and_the_hash_follows_it(tmp_path):
  """What tests/test_build_deps.py holds for the libraries of `build.LIBRARIES`, for this one: `deps` names the project's files
  `hipcc -MM` reads, and the hash moves with each of them and with no file of another library."""
  import shutil
  lib = build.library('rocks')
  keep = [f for f in lib.flags if f not in ('-shared', '-fPIC')]
  mm = subprocess.run([HIPCC] + keep + ['--cuda-host-only', '-MM', '-w', os.path.join(build.CSRC, 'rocks.hip')], check=True,
                      stdout=subprocess.PIPE, universal_newlines=True).stdout
  files = re.sub(r'\\\n', ' ', mm).split(':', 1)[1].split()
  assert build.deps('rocks') == sorted(os.path.relpath(os.path.realpath(f), os.path.realpath(build.ROOT)) for f in files)
  for d in build.deps('rocks') + build.deps('compare'):
    os.makedirs(os.path.dirname(str(tmp_path / d)), exist_ok=True)
    shutil.copy(os.path.join(build.ROOT, d), str(tmp_path / d))
  root = str(tmp_path)
  assert build.source_hash('rocks', root) == build.source_hash('rocks')
  for d in build.deps('rocks'):
    before = build.source_hash('rocks', root)
    with open(os.path.join(root, d), 'ab') as f:
      f.write(b'\n')
    assert build.source_hash('rocks', root) != before, d
  before = build.source_hash('rocks', root)
  with open(os.path.join(root, 'stackrl_amd', 'csrc', 'compare.hip'), 'ab') as f:
    f.write(b'\n')
  assert build.source_hash('rocks', root) == before


def test_points_per_subdivision_and_its_refusals():
  from stackrl_amd import rocks
  lib = rocks.load()
  n = ctypes.c_int32(-1)
  for s, want in enumerate((8, 26, 98, 386)):
    assert lib.srl_rocks_points(s, ctypes.byref(n)) == 0 and n.value == want == rocks.n_points(s)
  for s in (-1, 4):
    assert lib.srl_rocks_points(s, ctypes.byref(n)) == 1 and 'subdivisions must be in 0..3' in lib.srl_rocks_last_error().decode()
  assert lib.srl_rocks_points(0, None) == 1 and 'n_points is null' in lib.srl_rocks_last_error().decode()


def test_each_refusal_has_its_own_text_and_launches_nothing():
  """The refusals return before any HIP call, so they can be taken on a machine without a device: the pointers are never
  dereferenced (1 stands for a non-null device pointer)."""
  from stackrl_amd import rocks
  lib = rocks.load()

  def params(**kw):
    q = dict(radius=0.0625, irregularity=0.5, extents=(1.0, 0.5, 1 / 3), subdivisions=3, density_lo=2200.0, density_hi=2600.0, fit=0, seed=11)
    q.update(kw)
    return rocks.Params(q['radius'], q['irregularity'], (ctypes.c_float * 3)(*q['extents']), q['subdivisions'], q['density_lo'],
                        q['density_hi'], q['fit'], q['seed'])

  def refused(p, n=1, points_in=None, n_points_in=0, outputs=(1,) * 9):
    rc = lib.srl_rocks_generate(ctypes.byref(p) if p is not None else None, 0, n, points_in, n_points_in, None, *outputs, None)
    assert rc == 1
    return lib.srl_rocks_last_error().decode()

  texts = [refused(None), refused(params(), n=0), refused(params(subdivisions=4)), refused(params(subdivisions=-1)),
           refused(params(irregularity=0.0)), refused(params(irregularity=1.5)), refused(params(irregularity=float('nan'))),
           refused(params(), points_in=1, n_points_in=3), refused(params(), points_in=1, n_points_in=387),
           refused(params(radius=0.0)), refused(params(fit=2))]
  assert 'parameters are null' in texts[0]
  assert 'n must be at least 1, got 0' in texts[1]
  assert 'subdivisions must be in 0..3, got 4' in texts[2] and 'got -1' in texts[3]
  assert all('irregularity must be in (0, 1]' in t for t in texts[4:7])
  assert 'must number 4..386 a rock, got 3' in texts[7] and 'got 387' in texts[8]
  assert all('radius and extents must be positive' in t for t in texts[9:])
  for k in range(9):                                # each required output in turn
    out = [1] * 9
    out[k] = None
    assert 'a required output pointer is null' in refused(params(), outputs=tuple(out))
  # with points given, the irregularity is not read
  assert 'must number' in refused(params(irregularity=0.0), points_in=1, n_points_in=2)
  assert len({t.split(',')[0] for t in texts}) >= 6


def test_no_kernel_of_the_library_contains_the_flagged_packed_form():
  text = build.device_asm(HIPCC, build.QFLAGS, os.path.join(build.CSRC, 'rocks.hip'))
  assert not isa_fix.flagged(text)
  assert 'k_rocks' in text and text.count('v_mul_f64') > 100                                   # the scan saw the kernel
  build.build()
  texts = isa_fix.shipped_asm(build.RLIB)
  assert len(texts) == 1 and not isa_fix.flagged(texts[0])
  assert 'k_rocks' in texts[0] and texts[0].count('v_mul_f64') > 100
