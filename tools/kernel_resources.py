#!/usr/bin/env python3
"""Registers, spills, scratch and instruction count of every kernel of a library, from its compiled device assembly.

usage: kernel_resources.py [env|qnet|compare|rocks|valueview|candidates] [--dump DIR]

The library's sources are compiled to gfx950 assembly with its own flags (build.LIBRARIES, build.device_asm); the env library's
text then goes through isa_fix.rewrite, as in the product build.  No GPU needed.  With --dump every kernel's instruction text
(from its label to its end, labels renumbered in order of appearance) is written to DIR/<kernel>.s, so that two commits can be
compared with diff: a kernel whose text is the same runs the same instructions."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stackrl_amd import build, isa_fix

FIELDS = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size')
_META = re.compile(r'^(?:  - |    )\.(\w+):\s*(\S+)\s*$')      # a kernel's own keys (its arguments' sit deeper)
_LABEL = re.compile(r'\.L[A-Za-z_]*\d+(?:_\d+)?')


def metadata(text):
  """{kernel: {field: value}} from the assembly's amdgpu_metadata."""
  out, cur = {}, None
  for line in text[text.find('amdhsa.kernels:'):].splitlines():
    if line.startswith('  - '):
      cur = {}
    m = _META.match(line)
    if m and cur is not None:
      cur[m.group(1)] = m.group(2)
      if m.group(1) == 'name':
        out[m.group(2)] = cur
  return out


def body(text, kernel):
  """The lines between the kernel's label and its end: instructions and local labels, comments stripped, local labels
  renumbered in order of appearance."""
  lines = text.split('\n')
  i = next(k for k, line in enumerate(lines) if line.split(';')[0].rstrip() == kernel + ':')
  out, names = [], {}
  for line in lines[i + 1:]:
    if line.startswith('.Lfunc_end'):
      break
    line = line.split(';')[0].rstrip()
    if not line.strip() or (line.lstrip().startswith('.') and not line.startswith('.L')):
      continue
    out.append(_LABEL.sub(lambda m: names.setdefault(m.group(0), '.L%d' % len(names)), line))
  return out


def main(argv):
  dump = None
  if '--dump' in argv:
    i = argv.index('--dump'); dump = argv[i + 1]; argv = argv[:i] + argv[i + 2:]
  name = argv[0] if argv else 'env'
  lib = build.LIBRARIES[name]
  hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
  if dump:
    os.makedirs(dump, exist_ok=True)
  print('{:<40}'.format('kernel') + ''.join('{:>28}'.format(f) for f in FIELDS) + '{:>14}'.format('instructions'))
  for src in lib.sources:
    text = build.device_asm(hipcc, lib.flags, os.path.join(build.CSRC, src))
    if name == 'env':
      text = isa_fix.rewrite(text)[0]
    for kernel, md in sorted(metadata(text).items()):
      b = body(text, kernel)
      print('{:<40}'.format(kernel) + ''.join('{:>28}'.format(md.get(f, '-')) for f in FIELDS) +
            '{:>14}'.format(sum(1 for l in b if l[0].isspace())))
      if dump:
        with open(os.path.join(dump, kernel + '.s'), 'w') as f:
          f.write('\n'.join(b) + '\n')


if __name__ == '__main__':
  main(sys.argv[1:])
