"""Builds the native libraries in-tree with hipcc for gfx950 (no JIT cache: the .so files travel with the tree).

`LIBRARIES` says what differs between them; what a library depends on is read from its sources' `#include "..."` lines
(`deps`), and one `source_hash`, `stale` and `build_library` serve them all."""
import os
import re
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libstackrl_hip.so')
QLIB = os.path.join(HERE, 'libstackrl_qnet.so')
CLIB = os.path.join(HERE, 'libstackrl_compare.so')
RLIB = os.path.join(HERE, 'libstackrl_rocks.so')
VLIB = os.path.join(HERE, 'libstackrl_valueview.so')
KLIB = os.path.join(HERE, 'libstackrl_candidates.so')
_BASE = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared']
_WARN = ['-Wall', '-Wno-unused-function', '-Wno-unused-value', '-Wno-unused-result']
# -ffp-contract=off: the solver/rasteriser definition is "one IEEE rounding per written operation"
# The packed-fp32 erratum: on the MI355X boxes of this pool a v_pk_add_f32 / v_pk_mul_f32 whose LOW lane
#   takes the HIGH half of its SECOND source (op_sel:[x,1]; v_pk_fma_f32 too, and its addend) reads 0 for that operand now and
#   then while another wavefront on the CU issues one of gfx950's MFMA shapes with 128-bit A / B operands
#   (v_mfma_f32_16x16x32_bf16 / _f16, v_mfma_f32_32x32x16_bf16, v_mfma_i32_16x16x64_i8): measured with a 30-line victim
#   (tools/experiments/pk_seq2.hip) beside one-property aggressors (tools/experiments/pk_aggressor.hip, tools/diag_aggressor.py,
#   profiles/r04_erratum_aggressor*.log) — 1 - 3 % of the executions beside a bare loop of such MFMAs, whether their
#   accumulators live in v or a registers, at any s_setprio, with or without wait states between them; 0 beside
#   v_mfma_f32_16x16x4_f32, the 64-bit-operand v_mfma_f32_16x16x16_bf16, vector FMAs, DPP, v_perm_b32, SDWA or packed FMAs, and
#   0 alone.  clang's SLP vectoriser emits exactly that form when it packs scalars that sit in different halves of their
#   pairs; with it the settle and render kernels returned results that differ from the oracle's in a few envs per thousand
#   steps, only beside the Q-net's bf16 convolution kernels.  The env library is therefore built in steps: device assembly
#   (vectoriser on: it is worth 3.4 % of the settle kernel), `isa_fix.rewrite` (the two commuting sources of every flagged
#   instruction swapped — the same selection on the FIRST source is clean), assembler, code object, fat binary, host object,
#   link: what hipcc does in one go, with the pass in the middle.  If any step fails the library is built in one go WITHOUT
#   the vectoriser instead (FLAGS_SAFE: no flagged instruction either, slower); the library says which it is
#   (`srl_build_info`, printed by bench.py).  tests/test_isa_guard.py checks the compiled ISA of every source file of all
#   libraries AND disassembles the shipped .so files.
FLAGS = _BASE + ['-ffp-contract=off', '-fno-fast-math'] + _WARN
FLAGS = FLAGS + os.environ.get('SRL_EXTRA_FLAGS', '').split()      # experiments only (e.g. -DSRL_STAMPS)
FLAGS_SAFE = FLAGS + ['-fno-slp-vectorize']
# the Q-net ops are ordinary fp32 kernels compared against a torch fp32 reference with a stated tolerance
# (-fno-slp-vectorize: see above; it costs the Q-net's kernels nothing measurable — 20.6 against 20.8 ms per 2,048-sample forward)
QFLAGS = _BASE + ['-fno-slp-vectorize'] + _WARN
LLVM_BIN = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin')
VARIANT_FIXED = 'vectorised+rewritten'     # SLP vectoriser on, isa_fix.rewrite over the assembly
VARIANT_SAFE = 'safe'                      # one go without the SLP vectoriser (the fall-back; ~3 % slower settle kernel)


INFO_MARK = b'SRL_BUILD_INFO<'


def info(path):
  """What a built library says about itself — {'variant': ..., 'hash': ...} — read from the bytes of the file (the string
  `srl_build_info()` returns), or None for a file without it.  `stale` compares the hash with the sources'."""
  try:
    with open(path, 'rb') as f:
      data = f.read()
  except OSError:
    return None
  i = data.find(INFO_MARK)
  if i < 0:
    return None
  j = data.find(b'>', i)
  variant, _, digest = data[i + len(INFO_MARK):j].decode().partition('|')
  return {'variant': variant, 'hash': digest}


def _info_flag(variant, digest):
  return '-DSRL_BUILD_INFO="{}{}|{}>"'.format(INFO_MARK.decode(), variant, digest)


def device_asm(hipcc, flags, src):
  """gfx950 assembly of one source file, compiled with `flags` (no GPU needed)."""
  keep = [f for f in flags if f not in ('-shared', '-fPIC')]
  return subprocess.run([hipcc] + keep + ['--cuda-device-only', '-S', '-w', '-o', '-', src], check=True,
                        stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, universal_newlines=True).stdout


def fixed_env_asm(hipcc):
  """The env library's device assembly after the rewrite; raises if a flagged instruction is left."""
  from stackrl_amd import isa_fix
  text, n, left = isa_fix.rewrite(device_asm(hipcc, FLAGS, os.path.join(CSRC, LIBRARIES['env'].sources[0])))
  bad = isa_fix.flagged(text)
  if left or bad:
    raise RuntimeError('{} packed instructions of the failing form could not be rewritten: {}'.format(left or len(bad), bad[:3]))
  return text, n


def _run(cmd, verbose):
  if verbose:
    print(' '.join(cmd), file=sys.stderr)
  subprocess.run(cmd, check=True, stdout=None if verbose else subprocess.DEVNULL)


def _hipcc_once(lib, hipcc, digest, out, verbose, flags=None, variant=None):
  """One hipcc command from the sources to the library."""
  _run([hipcc] + (flags or lib.flags) + [_info_flag(variant or lib.variants[0], digest)] +
       [os.path.join(CSRC, s) for s in lib.sources] + ['-o', out], verbose)


def _env_fixed(lib, hipcc, digest, out, verbose):
  import tempfile
  src = os.path.join(CSRC, lib.sources[0])
  with tempfile.TemporaryDirectory() as tmp:
    text, n = fixed_env_asm(hipcc)
    asm, obj, co, fb, host = (os.path.join(tmp, f) for f in ('dev.s', 'dev.o', 'dev.out', 'dev.hipfb', 'host.o'))
    with open(asm, 'w') as f:
      f.write(text)
    for cmd in (
        [os.path.join(LLVM_BIN, 'clang'), '-x', 'assembler', '-target', 'amdgcn-amd-amdhsa', '-mcpu=gfx950', '-c', asm, '-o', obj],
        [os.path.join(LLVM_BIN, 'lld'), '-flavor', 'gnu', '-m', 'elf64_amdgpu', '--no-undefined', '-shared', '-o', co, obj],
        [os.path.join(LLVM_BIN, 'clang-offload-bundler'), '-type=o', '-bundle-align=4096',
         '-targets=host-x86_64-unknown-linux-gnu,hipv4-amdgcn-amd-amdhsa--gfx950', '-input=/dev/null', '-input=' + co, '-output=' + fb],
        [hipcc] + [f for f in lib.flags if f != '-shared'] + [_info_flag(VARIANT_FIXED, digest), '--cuda-host-only',
                                                             '-Xclang', '-fcuda-include-gpubinary', '-Xclang', fb, '-c', src, '-o', host],
        [hipcc, '-shared', '-fPIC', host, '-o', out + '.tmp']):
      _run(cmd, verbose)
    os.replace(out + '.tmp', out)
  if verbose:
    print('env library: {} packed instructions rewritten'.format(n), file=sys.stderr)


def _env_pipeline(lib, hipcc, digest, out, verbose):
  """The env library the long way round (see above), or in one go without the vectoriser if a step of it fails."""
  try:
    if os.environ.get('SRL_BUILD_SAFE'):
      raise RuntimeError('SRL_BUILD_SAFE is set')
    _env_fixed(lib, hipcc, digest, out, verbose)
  except Exception as e:         # any step of the long way round: the plain build without the vectoriser (same results, slower)
    print('stackrl_amd.build: env library built without the SLP vectoriser ({})'.format(str(e)[:200]), file=sys.stderr)
    _hipcc_once(lib, hipcc, digest, out, verbose, FLAGS_SAFE, VARIANT_SAFE)


def _library(path, sources, flags, variants, compile=_hipcc_once, recipe=()):
  return types.SimpleNamespace(path=path, sources=sources, flags=flags, variants=variants, compile=compile, recipe=list(recipe))


# What differs between the libraries.  `path` is read when a library is loaded or built, so a diagnostic points a library at
# another file by assigning it before first use.  `variants`: what `info(path)['variant']` may say, the product's first.
# `recipe`: files (relative to the repository) that shape the library besides its sources and belong in its hash.
LIBRARIES = {
  'env': _library(LIB, ['stackrl_hip.hip'], FLAGS, (VARIANT_FIXED, VARIANT_SAFE), _env_pipeline,
                  [os.path.join('stackrl_amd', 'isa_fix.py'), os.path.join('stackrl_amd', 'build.py')]),
  'qnet': _library(QLIB, ['qnet.hip', 'greedy.hip', 'heuristics.hip', 'xcorr_mfma.hip', 'epilogue.hip', 'conv_mfma.hip',
                          'conv_gemm.hip', 'learner.hip', 'train_conv.hip'], QFLAGS, ('no-slp',)),
  # the policy-comparison statistics (include/stackrl_compare.h): a library of its own, so that libstackrl_qnet.so keeps its exports
  'compare': _library(CLIB, ['compare.hip'], QFLAGS, ('no-slp',)),
  # off the training path, each a library of its own like `compare`: the procedural rock generator (include/stackrl_rocks.h),
  'rocks': _library(RLIB, ['rocks.hip'], QFLAGS, ('no-slp',)),
  # the frames of a visualised comparison run (include/stackrl_valueview.h),
  'valueview': _library(VLIB, ['valueview.hip'], QFLAGS, ('no-slp',)),
  # and the spread candidates of a lookahead (include/stackrl_candidates.h)
  'candidates': _library(KLIB, ['candidates.hip'], QFLAGS, ('no-slp',)),
}
QSRC = LIBRARIES['qnet'].sources


_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def deps(name, root=ROOT):
  """The files library `name` is built from, relative to `root` (the repository, or a copy of it) and sorted: its sources,
  whatever they reach through `#include "..."` lines (each resolved against the including file), and its recipe files."""
  lib = LIBRARIES[name]
  seen, todo = set(lib.recipe), [os.path.join('stackrl_amd', 'csrc', s) for s in lib.sources]
  while todo:
    d = todo.pop()
    if d not in seen:
      seen.add(d)
      with open(os.path.join(root, d)) as f:
        todo += [os.path.normpath(os.path.join(os.path.dirname(d), i)) for i in _INCLUDE.findall(f.read())]
  return sorted(seen)


def source_hash(name, root=ROOT):
  """sha256 over the contents of the files library `name` is built from and the flags it is built with (first 16 hex digits)."""
  import hashlib
  h = hashlib.sha256()
  for d in deps(name, root):
    with open(os.path.join(root, d), 'rb') as f:
      h.update(d.encode() + b'\0' + f.read() + b'\0')
  h.update(' '.join(LIBRARIES[name].flags).encode())
  return h.hexdigest()[:16]


def stale(name):
  """The library is missing, or was not built from these sources with these flags (the hash it carries, not file times)."""
  i = info(LIBRARIES[name].path)
  return i is None or i['hash'] != source_hash(name)


def build_library(name, out=None, verbose=False):
  """Build library `name` to `out` (default: its place in the tree)."""
  lib = LIBRARIES[name]
  lib.compile(lib, os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), source_hash(name), out or lib.path, verbose)


def build(force=False, verbose=False):
  """Build every library that is missing or stale (all of them with `force`); returns the env library's path."""
  for name in LIBRARIES:
    if force or stale(name):
      build_library(name, verbose=verbose)
  return LIBRARIES['env'].path


if __name__ == '__main__':
  build(force='-f' in sys.argv, verbose=True)
