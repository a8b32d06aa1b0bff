"""CPU tests of what only libstackrl_rocks.so has at its boundary: `rocks.Params` held to the header's struct field by field,
the limits, the points of a subdivision, and its refusals (each with a text of its own, none of which launches anything).  The
boundary it shares with the other libraries is held in tests/test_abi.py, tests/test_build_deps.py and tests/test_isa_guard.py."""
import ctypes
import re

import library_boundary as boundary


def test_parameter_struct_and_limits_are_the_headers():
  from stackrl_amd import rocks
  # the parameter struct, field by field
  header = boundary.header_text('stackrl_rocks.h')
  body = re.search(r'typedef struct srl_rocks_params \{(.*?)\}\s*srl_rocks_params;', header, re.S).group(1)
  fields = []
  for typ, names in re.findall(r'(\w+)\s+([^;]+);', body):
    for n in names.split(','):
      m = re.match(r'\s*(\w+)(?:\[(\d+)\])?\s*$', n)
      fields.append((m.group(1), boundary.ctype(typ) * int(m.group(2)) if m.group(2) else boundary.ctype(typ)))
  assert [(n, t) for n, t in rocks.Params._fields_] == fields and ctypes.sizeof(rocks.Params) == 40
  # the limits are the env's
  assert (rocks.MAX_VERTS, rocks.MAX_TRIS, rocks.MAX_POINTS) == (128, 252, 386)


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
