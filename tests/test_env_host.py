"""The env library's host arithmetic (stackrl_amd/csrc/env_host.h: mesh table, refusals, layouts, variant choice) on a CPU:
tests/host/env_host_main.hip holds the checks; here it is built with the project's compiler, its host code under
AddressSanitizer and UndefinedBehaviorSanitizer, linked as an ordinary executable and run as a child process.  The program
makes no HIP runtime call, so it opens no device; nothing is preloaded.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SANITIZE = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all']


@pytest.fixture(scope='module')
def program(tmp_path_factory):
  exe = str(tmp_path_factory.mktemp('env_host') / 'env_host_main')
  subprocess.run([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-Wall', '-Wno-unused-function'] + SANITIZE +
                 [os.path.join(ROOT, 'tests', 'host', 'env_host_main.hip'), '-o', exe], check=True)
  return exe


def test_the_program_carries_both_sanitizers(program):
  with open(program, 'rb') as f:
    data = f.read()
  assert b'__asan_init' in data and b'__ubsan_handle' in data


def test_mesh_table_refusals_and_layouts_under_the_sanitizers(program):
  env = dict(os.environ)
  env.pop('SRL_STEP_VARIANT', None)      # (the variant rows are checked as the batch size chooses them)
  r = subprocess.run([program], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
  print(r.stdout)
  print(r.stderr)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
  assert r.stdout.rstrip().endswith('env_host: ok')
  assert 'MISMATCH' not in r.stdout
  for mark in ('Sanitizer', 'runtime error'):       # no report from either
    assert mark not in r.stderr and mark not in r.stdout
