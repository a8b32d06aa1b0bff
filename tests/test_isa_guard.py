"""No kernel of any library may contain the packed-fp32 instruction form that misreads an operand on gfx950.

Found in round 3, its trigger narrowed down in round 4 (tools/experiments/pk_seq2.hip is the 30-line
victim, tools/experiments/pk_aggressor.hip the one-property aggressors): a packed-fp32 instruction whose LOW lane takes the HIGH
half of its SECOND source — `v_pk_add_f32` / `v_pk_mul_f32` / `v_pk_fma_f32` with `op_sel:[x,1...]`, and the fma's addend likewise
(`op_sel:[x,x,1]`) — reads 0 for that operand in 1 - 3 % of its executions while another wavefront of the CU runs a loop of
gfx950's 128-bit-operand MFMA shapes (`v_mfma_f32_16x16x32_bf16` / `_f16`, `_32x32x16_bf16`, `v_mfma_i32_16x16x64_i8`; 2 - 4 per
10,000 beside the Q-net's bf16 convolution kernels), and never alone, beside fp32 or 64-bit-operand MFMAs, or beside vector-ALU
work.  clang's SLP vectoriser emits the form.  The env library is compiled with the vectoriser and a pass over its assembly
that swaps the two (commuting) sources of every such instruction (stackrl_amd/isa_fix.py; the same selection on the first
source is clean); the other libraries are built without the vectoriser.  These tests compile every source to gfx950 assembly
the way stackrl_amd/build.py does AND take the shipped .so files apart (no GPU needed), so that a later flag, compiler or
source change — or a stale library — cannot bring the form back unnoticed."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

from stackrl_amd import build, isa_fix

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def _packed(text, variant):
  return text.count('v_pk_') > (1000 if variant == build.VARIANT_FIXED else 50)


# "the scan saw real code", per library: (on the compiled assembly, on the disassembly of the shipped library), each
# (all of the library's text, variant) -> bool
_SAW = {
  # the env kernels: the vectorised library is full of packed instructions, the ray cast's hand-written ones (halves of the
  # FIRST source only) are in the fall-back build too; in the shipped library the step and render kernels by name
  'env': (_packed, lambda text, variant: _packed(text, variant) and '<srl_k_step>:' in text and '<srl_k_render>:' in text),
  'qnet': (lambda text, variant: text.count('v_mfma_') > 1000,) * 2,
  # nothing of the shipped kernels spills to memory (P = 8: 36 float64 sums and 72 counts a thread)
  'compare': (lambda text, variant: text.count('k_compare') >= 8 and 'k_fold' in text and 'v_fma_f64' in text,
              lambda text, variant: text.count('k_compare') >= 8 and 'v_fma_f64' in text and 'scratch_' not in text),
  'rocks': (lambda text, variant: 'k_rocks' in text and text.count('v_mul_f64') > 100,) * 2,
  'valueview': (lambda text, variant: 'k_value_range' in text and 'k_value_frame' in text and text.count('v_div_fixup_f32') >= 1,) * 2,
  'candidates': (lambda text, variant: text.count('k_candidates') >= 2 and text.count('s_barrier') >= 4,) * 2,      # both kernels
}


def test_no_kernel_contains_the_packed_form_that_fails_beside_wide_operand_mfma_wavefronts():
  env = build.LIBRARIES['env']
  jobs = [('env', build.VARIANT_FIXED, lambda: build.fixed_env_asm(HIPCC)[0]),                         # the product's env library
          ('env', build.VARIANT_SAFE, lambda: build.device_asm(HIPCC, build.FLAGS_SAFE, os.path.join(build.CSRC, env.sources[0])))]
  for name, lib in build.LIBRARIES.items():        # every other library: each source, the way its one command compiles it
    if lib is not env:
      jobs += [(name, lib.variants[0], lambda s=s, lib=lib: build.device_asm(HIPCC, lib.flags, os.path.join(build.CSRC, s)))
               for s in lib.sources]
  with ThreadPoolExecutor(max_workers=6) as ex:
    texts = list(ex.map(lambda job: job[2](), jobs))
  seen = {}
  for (name, variant, _), text in zip(jobs, texts):
    hits = isa_fix.flagged(text)
    assert not hits, '{} ({}): packed instructions that take the high half of their second source for the low lane: {}'.format(
        name, variant, hits[:5])
    seen.setdefault((name, variant), []).append(text)
  assert sorted({name for name, _ in seen}) == sorted(_SAW)
  for (name, variant), group in seen.items():      # the scan saw real code
    assert _SAW[name][0]('\n'.join(group), variant), (name, variant)


def test_the_shipped_libraries_are_built_from_these_sources_and_contain_no_flagged_instruction():
  """The ARTEFACTS, not the recipe: every .so file that travels to the GPU box is taken apart (`.hip_fatbin` section ->
  the gfx950 code object of every translation unit -> llvm-objdump) and scanned; the hash each carries (`srl_build_info`)
  must be that of the sources and flags in the tree, so a stale or hand-copied library fails here; and the env library
  says which variant it is (the bench line prints it)."""
  build.build()                                   # a no-op unless a library is missing or stale
  assert sorted(_SAW) == sorted(build.LIBRARIES)  # a new library comes with its own "saw real code" count
  for name, lib in build.LIBRARIES.items():
    i = build.info(lib.path)
    assert i is not None and i['hash'] == build.source_hash(name), '{} was not built from the sources in the tree'.format(lib.path)
    assert i['variant'] in lib.variants
    texts = isa_fix.shipped_asm(lib.path)
    assert len(texts) == len(lib.sources)
    for t in texts:
      hits = isa_fix.flagged(t)
      assert not hits, '{}: {}'.format(os.path.basename(lib.path), hits[:5])
    assert _SAW[name][1]('\n'.join(texts), i['variant']), name


def test_the_vectoriser_does_emit_the_form_and_the_pass_removes_all_of_it():
  raw = build.device_asm(HIPCC, build.FLAGS, os.path.join(build.CSRC, build.LIBRARIES['env'].sources[0]))
  assert len(isa_fix.flagged(raw)) > 100          # (955 with the compiler of this image)
  text, n, left = isa_fix.rewrite(raw)
  assert n == len(isa_fix.flagged(raw)) and left == 0 and not isa_fix.flagged(text)
  # nothing but the flagged lines changes, and the rewritten text is the per-line fixes in their places and order
  fixed = [isa_fix._fix(l)[0] for l in raw.split('\n')]
  assert text == '\n'.join(fixed)
  changed = [(a, b) for a, b in zip(raw.split('\n'), fixed) if a != b]
  assert len(changed) == n and all(isa_fix.BAD.match(a) for a, _ in changed)
  # a split adds one line (two with the crosswise swap); a swap adds none
  added = sum(b.count('\n') for _, b in changed)
  assert len(text.split('\n')) == len(raw.split('\n')) + added
  assert added == sum(1 + ('v_swap_b32' in b) for _, b in changed if '\n' in b)


def test_the_rewrite_swaps_sources_and_modifier_bits():
  f = isa_fix._fix
  assert f('\tv_pk_add_f32 v[34:35], v[0:1], v[32:33] op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]') == \
      ('\tv_pk_add_f32 v[34:35], v[32:33], v[0:1] op_sel:[1,0] op_sel_hi:[0,1] neg_lo:[1,0] neg_hi:[1,0]', True)
  assert f('\tv_pk_fma_f32 v[114:115], v[112:113], s[4:5], v[114:115] op_sel:[0,1,0] ; c') == \
      ('\tv_pk_fma_f32 v[114:115], s[4:5], v[112:113], v[114:115] op_sel:[1,0,0] ; c', True)
  assert f('\tv_pk_mul_f32 v[2:3], v[2:3], v[8:9] op_sel:[0,1]')[0] == '\tv_pk_mul_f32 v[2:3], v[8:9], v[2:3] op_sel:[1,0]'
  # a swap cannot help where both sources (or the fma's addend) select the high half for the low lane: the instruction is
  # written as its two lanes, ordered so that neither overwrites what the other still reads
  assert f('\tv_pk_mul_f32 v[34:35], v[0:1], v[32:33] op_sel:[1,1]') == \
      ('\tv_mul_f32_e64 v34, v1, v33 ; isa_fix: split of v_pk_mul_f32 v[34:35], v[0:1], v[32:33] op_sel:[1,1]\n\tv_mul_f32_e64 v35, v1, v33', True)
  # each lane's destination is the other lane's source (the shape the compiler emits in the settle kernels): crosswise + swap
  assert f('\tv_pk_mul_f32 v[78:79], v[78:79], v[80:81] op_sel:[1,1] op_sel_hi:[0,1]')[0].split('\n')[1:] == \
      ['\tv_mul_f32_e64 v79, v79, v81', '\tv_swap_b32 v78, v79']
  assert f('\tv_pk_mul_f32 v[78:79], v[78:79], v[80:81] op_sel:[1,1] op_sel_hi:[0,1]')[0].startswith('\tv_mul_f32_e64 v78, v78, v81 ;')
  bad_addend = '\tv_pk_fma_f32 v[34:35], v[0:1], v[0:1], v[32:33] op_sel:[0,0,1] op_sel_hi:[1,1,0]'    # the addend fails as well
  assert isa_fix.BAD.match(bad_addend) and f(bad_addend)[1] is True and not isa_fix.flagged(f(bad_addend)[0])
  assert f(bad_addend)[0].split('\n')[1] == '\tv_fma_f32 v35, v1, v1, v32' and ' v34, v0, v0, v33 ;' in f(bad_addend)[0]
  # high lane first where the low lane's destination is a source of the high lane
  hf = f('\tv_pk_fma_f32 v[0:1], v[0:1], v[4:5], v[6:7] op_sel:[0,0,1] op_sel_hi:[0,1,0] neg_lo:[0,1,0]')[0].split('\n')
  assert hf[0].startswith('\tv_fma_f32 v1, v0, v5, v6 ;') and hf[1:] == ['\tv_fma_f32 v0, v0, -v4, v7']
  cw = f('\tv_pk_add_f32 v[0:1], v[0:1], v[4:5] op_sel:[1,1] op_sel_hi:[0,0] neg_lo:[0,1]')[0].split('\n')
  assert cw[0].startswith('\tv_add_f32_e64 v0, v0, v4 ;') and cw[1:] == ['\tv_add_f32_e64 v1, v1, -v5', '\tv_swap_b32 v0, v1']
  # operands the split does not express are reported (build.py then builds without the vectoriser)
  sgpr = '\tv_pk_mul_f32 v[34:35], s[0:1], v[32:33] op_sel:[1,1]'
  assert f(sgpr)[1] is None and isa_fix.rewrite(sgpr)[2] == 1
  for clean in ('\tv_pk_fma_f32 v[8:9], v[6:7], v[24:25], v[8:9] op_sel:[1,0,0] op_sel_hi:[1,1,0]',    # first source only
                '\tv_pk_mul_f32 v[8:9], v[20:21], v[8:9] op_sel_hi:[0,1]',
                '\tv_pk_add_f32 v[50:51], v[52:53], v[50:51] neg_lo:[0,1] neg_hi:[0,1]',
                '\tv_add_f32_e32 v1, v2, v3'):
    assert f(clean) == (clean, False) and not isa_fix.BAD.match(clean)


# ------------------------------------------------------------------------------------------------ LDS read windows
# The settle kernels issue `ds_read_b128` from inline asm (settle.hip cg_request / cg_request_first) into "=&v" outputs
# that hold the data only from the hand-written `s_waitcnt lgkmcnt(k)` of cg_arrive on: the compiler takes the registers
# as written when the asm statement ends.  A copy or spill of those registers in between would read them before the data
# arrives.  So, in the disassembly of the shipped settle kernels, every `ds_read_b128` has a window that runs up to the first
# wait that retires it — `lgkmcnt(k)` with k <= the LDS operations issued after the read (LDS operations return in order;
# scalar loads do not, and count as none here, which can only lengthen a window) — and in it no instruction names one of
# the read's destination registers, and no branch leaves or enters it (DESIGN: every read is waited for in the block that
# issued it).
SETTLE_KERNELS = ('srl_k_step', 'srl_k_step_pp1', 'srl_k_step_pp2', 'srl_k_step_t128')
_FUNC = re.compile(r'^([0-9a-f]+) <([^>]+)>:$')
_LINE = re.compile(r'^\s+([a-z_0-9]+)\b([^/]*)(?://\s*([0-9A-Fa-f]+):[^<]*(?:<([^>+]+)\+0x([0-9a-f]+)>)?)?')
_VREG = re.compile(r'(?<![\w\[])v(\d+)\b|(?<![\w\[])v\[(\d+):(\d+)\]')
_LGKM = re.compile(r'lgkmcnt\((\d+)\)')
_BRANCH = ('s_branch', 's_cbranch_', 's_setpc_', 's_swappc_', 's_endpgm', 's_call_')


def _vregs(operands):
  out = set()
  for m in _VREG.finditer(operands):
    if m.group(1) is not None:
      out.add(int(m.group(1)))
    else:
      out.update(range(int(m.group(2)), int(m.group(3)) + 1))
  return out


def _functions(text):
  """{name: [(address, mnemonic, operands, branch target address or None)]} of an `llvm-objdump -d` text."""
  funcs, cur, base = {}, None, 0
  for line in text.splitlines():
    m = _FUNC.match(line)
    if m:
      base, cur = int(m.group(1), 16), m.group(2)
      funcs[cur] = []
      continue
    m = _LINE.match(line)
    if cur is None or not m or m.group(3) is None:
      continue
    target = None
    if m.group(4) is not None:
      target = base + int(m.group(5), 16) if m.group(4) == cur else -1
    funcs[cur].append((int(m.group(3), 16), m.group(1), m.group(2).strip(), target))
  return funcs


def lds_window_violations(insns):
  """[(read address, problem)] of the `ds_read_b128` windows of one function's instruction list."""
  targets = {t for _, _, _, t in insns if t is not None}
  bad = []
  for i, (addr, op, opnds, _) in enumerate(insns):
    if op != 'ds_read_b128':
      continue
    dst = _vregs(opnds.split(',')[0])
    later_ds, closed = 0, False
    for addr2, op2, opnds2, _ in insns[i + 1:]:
      if op2 == 's_waitcnt':
        k = _LGKM.search(opnds2)
        if k and int(k.group(1)) <= later_ds:
          closed = True
          break
        continue
      if addr2 in targets:
        bad.append((addr, 'branch target {:#x} inside the window'.format(addr2)))
        break
      if op2.startswith(_BRANCH):
        bad.append((addr, '{} at {:#x} inside the window'.format(op2, addr2)))
        break
      if dst & _vregs(opnds2):
        bad.append((addr, '{} {} at {:#x} names a destination register before the wait'.format(op2, opnds2, addr2)))
        break
      if op2.startswith('ds_'):
        later_ds += 1
    else:
      if not closed:
        bad.append((addr, 'never waited for'))
  return bad


def settle_window_report(text):
  """{kernel: (ds_read_b128 count, violations)} of the settle kernels of one disassembly."""
  funcs = _functions(text)
  return {k: (sum(op == 'ds_read_b128' for _, op, _, _ in funcs[k]), lds_window_violations(funcs[k]))
          for k in SETTLE_KERNELS if k in funcs}


def test_lds_reads_of_the_settle_kernels_are_not_touched_before_their_wait():
  from stackrl_amd import build
  build.build()
  texts = isa_fix.shipped_asm(build.LIB)
  report = {}
  for t in texts:
    report.update(settle_window_report(t))
  assert sorted(report) == sorted(SETTLE_KERNELS)
  # the scan saw the hand-issued reads: the 128-thread variant requests a ground point's record ahead (seven reads a record)
  assert report['srl_k_step'][0] >= 28 and all(n > 0 for n, _ in report.values())
  for k, (n, bad) in report.items():
    assert not bad, '{}: {} of {} ds_read_b128 windows broken: {}'.format(k, len(bad), n, ['{:#x}: {}'.format(a, w) for a, w in bad[:5]])


_SYNTH = """0000000000001000 <srl_k_step>:
\tds_read_b128 v[10:13], v2 offset:16                         // 000000001000: D9FE0010 0A000002
\tds_read_b128 v[14:17], v2 offset:32                         // 000000001008: D9FE0020 0E000002
\tv_add_f32_e32 v20, v21, v22                                // 000000001010: 02282D15
\t{insn}
\ts_waitcnt lgkmcnt(1)                                        // 00000000101C: BF8C017F
\tv_mul_f32_e32 v30, v10, v11                                // 000000001020: 0A3C150A
\ts_waitcnt lgkmcnt(0)                                        // 000000001024: BF8C007F
\tv_mul_f32_e32 v31, v14, v17                                // 000000001028: 0A3E230E
\ts_endpgm                                                    // 00000000102C: BF810000
"""


def test_lds_window_check_flags_a_register_touched_before_its_wait():
  ok = _SYNTH.format(insn='v_mov_b32_e32 v40, v41                                     // 000000001014: 7E500329')
  assert lds_window_violations(_functions(ok)['srl_k_step']) == []
  # a copy of a destination register of the first read before lgkmcnt(1) retires it
  early = _SYNTH.format(insn='v_mov_b32_e32 v40, v12                                     // 000000001014: 7E50030C')
  bad = lds_window_violations(_functions(early)['srl_k_step'])
  assert [a for a, _ in bad] == [0x1000] and 'v_mov_b32_e32' in bad[0][1]
  # the second read is retired only by lgkmcnt(0): a use between the two waits is flagged, the same use after it is not
  late = _SYNTH.replace('v_mul_f32_e32 v30, v10, v11', 'v_mul_f32_e32 v30, v10, v15').format(insn='s_nop 0   // 000000001014: BF800000')
  assert [a for a, _ in lds_window_violations(_functions(late)['srl_k_step'])] == [0x1008]
  # a write to a destination register (a spill reload into it, say) is flagged as well, and so is a branch in the window
  w = _SYNTH.format(insn='v_mov_b32_e32 v16, 0                                       // 000000001014: 7E200280')
  assert [a for a, _ in lds_window_violations(_functions(w)['srl_k_step'])] == [0x1008]
  br = _SYNTH.format(insn='s_cbranch_scc1 3                                           // 000000001014: BF850003 <srl_k_step+0x24>')
  assert [a for a, _ in lds_window_violations(_functions(br)['srl_k_step'])] == [0x1000, 0x1008]
