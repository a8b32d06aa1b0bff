"""What a library is built from is derived (stackrl_amd/build.py `deps`: the sources, the closure of their quoted includes,
the recipe files), and its hash and `stale` follow that set.  The compiler is the reference for the set: `hipcc -MM` names the
files it reads for a source (tests/library_boundary.py `compiler_deps`).  No GPU needed."""
import itertools
import os
import shutil

import pytest

import library_boundary as boundary
from stackrl_amd import build

NAMES = sorted(build.LIBRARIES)


@pytest.mark.parametrize('name', NAMES)
def test_the_derived_set_is_the_compilers(name):
  assert build.deps(name) == boundary.compiler_deps(name)
  if name == 'env':
    assert os.path.join('stackrl_amd', 'csrc', 'stage.h') in build.deps('env')
    assert os.path.join('stackrl_amd', 'csrc', 'solver.h') in build.deps('env')


def test_no_two_libraries_share_a_file_but_the_types():
  """A library's sources, headers and recipe are its own: a change to one library's files rebuilds no other."""
  for a, b in itertools.combinations(NAMES, 2):
    assert set(build.deps(a)) & set(build.deps(b)) <= {boundary.TYPES}, (a, b)


def _copy(tmp_path):
  """The files of every library's set, copied to tmp_path at their places."""
  for d in {d for name in NAMES for d in build.deps(name)}:
    os.makedirs(os.path.dirname(str(tmp_path / d)), exist_ok=True)
    shutil.copy(os.path.join(build.ROOT, d), str(tmp_path / d))
  return str(tmp_path)


def test_the_hash_follows_every_file_of_the_set_and_no_other(tmp_path):
  root = _copy(tmp_path)
  for name in NAMES:
    assert build.deps(name, root) == build.deps(name)
    assert build.source_hash(name, root) == build.source_hash(name)       # the copy hashes like the tree
  for name in NAMES:
    for d in build.deps(name):
      before = build.source_hash(name, root)
      with open(os.path.join(root, d), 'ab') as f:
        f.write(b'\n')
      assert build.source_hash(name, root) != before, (name, d)
  # a file outside the set of every library but one
  before = {name: build.source_hash(name, root) for name in NAMES}
  with open(os.path.join(root, 'stackrl_amd', 'csrc', 'compare.hip'), 'ab') as f:
    f.write(b'\n')
  for name in NAMES:
    assert (build.source_hash(name, root) != before[name]) == (name == 'compare'), name


def test_after_a_build_no_library_is_stale():
  assert build.build() == build.LIB
  for name, lib in build.LIBRARIES.items():
    assert not build.stale(name)
    assert build.info(lib.path)['hash'] == build.source_hash(name)
