"""What a library is built from is derived (stackrl_amd/build.py `deps`: the sources, the closure of their quoted includes,
the recipe files), and its hash and `stale` follow that set.  The compiler is the reference for the set: `hipcc -MM` names the
files it reads for a source.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from stackrl_amd import build

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
NAMES = sorted(build.LIBRARIES)


def _compiler_deps(name):
  """The project's files that the compiler reads for the library's sources with the library's flags, relative to the
  repository, plus the recipe files."""
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


@pytest.mark.parametrize('name', NAMES)
def test_the_derived_set_is_the_compilers(name):
  assert build.deps(name) == _compiler_deps(name)
  if name == 'env':
    assert os.path.join('stackrl_amd', 'csrc', 'stage.h') in build.deps('env')
    assert os.path.join('stackrl_amd', 'csrc', 'solver.h') in build.deps('env')


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
  # a file outside the set
  before = {name: build.source_hash(name, root) for name in NAMES}
  with open(os.path.join(root, 'stackrl_amd', 'csrc', 'compare.hip'), 'ab') as f:
    f.write(b'\n')
  after = {name: build.source_hash(name, root) for name in NAMES}
  assert after['env'] == before['env'] and after['qnet'] == before['qnet'] and after['compare'] != before['compare']


def test_after_a_build_no_library_is_stale():
  assert build.build() == build.LIB
  for name, lib in build.LIBRARIES.items():
    assert not build.stale(name)
    assert build.info(lib.path)['hash'] == build.source_hash(name)
