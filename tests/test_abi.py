"""CPU tests of the boundary every native library keeps (no compute calls: there is no GPU here): the header(s), the ctypes
table and the exported symbols agree, and the library carries the hash of its sources, stated once over
`build.LIBRARIES` with what differs between the libraries in tests/library_boundary.py; then what only the env and the Q-net
library have.  The dependency sets are held in tests/test_build_deps.py and the packed-fp32 guard in tests/test_isa_guard.py."""
import ctypes
import os
import re

import pytest

import library_boundary as boundary
from stackrl_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(build.LIBRARIES)


@pytest.mark.parametrize('name', NAMES)
def test_header_table_and_exports_agree(name):
  """`_SIGS` names exactly the exports the headers declare, each with the declaration's return and argument types and the
  accessor of the row's rule; the library exports them, and its sources define each once."""
  row, sigs = boundary.ROWS[name], boundary.module(name)._SIGS
  build.build()                                   # a no-op unless a library is missing or stale
  decl = boundary.declarations(row.headers)
  assert sorted(sigs) == sorted(decl), 'ctypes signature table out of sync with the header'
  assert row.names is None or sorted(decl) == row.names
  assert row.build_info in decl and set(row.host_only) <= set(decl)
  for export, (ret, params) in decl.items():
    if row.untyped:
      continue
    assert sigs[export][0] is boundary.ctype(ret, ret=True), export
    assert list(sigs[export][1]) == [boundary.ctype(p) for p in params], export
    # the launching exports: the stream goes last (what `_bind.binding`'s `call` appends)
    assert (ret == 'int' and export not in row.host_only) == (''.join(params[-1:]).replace(' ', '') == 'void*stream'), export
    if row.accessor:
      assert sigs[export][2] == row.accessor(export, ret), export
  # the library exports these (and, without a reason for more, nothing else of the project's), each defined once in its sources
  exported, defined = boundary.exports(name), boundary.defined(name)
  assert set(decl) <= set(exported) and set(decl) <= set(defined)
  if not row.extra:
    assert exported == sorted(decl) == sorted(defined)
  assert all(ret == decl[export][0] for export, (_, ret) in defined.items() if export in decl)


@pytest.mark.parametrize('name', NAMES)
def test_library_carries_the_hash_of_its_sources(name):
  row, lib = boundary.ROWS[name], build.LIBRARIES[name]
  build.build()                                   # a no-op unless a library is missing or stale
  i = build.info(lib.path)
  assert i is not None and i['variant'] in lib.variants and i['hash'] == build.source_hash(name)
  assert not build.stale(name)
  said = getattr(boundary.module(name).load(), row.build_info)().decode()
  assert said == 'SRL_BUILD_INFO<{}|{}>'.format(i['variant'], i['hash'])
  # only the env library is compiled with the SLP vectoriser (and rewritten, or built the safe way)
  assert lib.flags is (build.FLAGS if name == 'env' else build.QFLAGS) and '-fno-slp-vectorize' in build.QFLAGS
  assert lib.variants == ((build.VARIANT_FIXED, build.VARIANT_SAFE) if name == 'env' else ('no-slp',))
  if row.deps is not None:                        # the hash follows the header(s) and the one source, named here
    assert build.deps(name) == row.deps and lib.sources == [os.path.basename(row.deps[-1])]


def test_library_builds_and_exports_every_declared_symbol():
  from stackrl_amd import lib
  path = build.build()
  assert os.path.isfile(path)
  L = ctypes.CDLL(path)
  names = sorted(boundary.declarations(boundary.ROWS['env'].headers))
  assert len(names) >= 18
  for n in names:
    assert hasattr(L, n), 'missing export ' + n
  assert sorted(lib.EXPORTS) == names, 'ctypes signature table out of sync with the header'


def test_qnet_library_exports_every_declared_symbol():
  build.build()
  names = sorted(boundary.declarations(('stackrl_qnet.h',)))
  assert names == ['srl_adam_step', 'srl_baseline_select', 'srl_bias_act', 'srl_bias_act_bwd_f32', 'srl_bias_act_bwd_scratch_floats', 'srl_bias_act_f32', 'srl_bias_act_pool', 'srl_bias_act_pool_f32', 'srl_conv3x3_bias_relu', 'srl_conv3x3_bias_relu_f32', 'srl_conv3x3_gemm_batch_multiple', 'srl_conv3x3_gemm_bias_relu', 'srl_conv3x3_gemm_supported', 'srl_conv3x3_gemm_wfrag_elems', 'srl_conv3x3_relu_project', 'srl_conv3x3_relu_project_f32', 'srl_conv3x3_thin', 'srl_conv3x3_thin_f32', 'srl_conv3x3_wfrag_elems', 'srl_conv_gemm_last_error',
                   'srl_conv_last_error', 'srl_convt2x2_bias_relu', 'srl_convt2x2_bias_relu_f32', 'srl_convt2x2_gemm_bias_relu', 'srl_convt2x2_gemm_supported', 'srl_convt2x2_wfrag_elems', 'srl_epilogue_last_error', 'srl_gumbel_topk',
                   'srl_gumbel_topk_scratch_bytes', 'srl_heuristic', 'srl_learner_last_error', 'srl_logit_extrema', 'srl_logit_extrema_scratch_bytes',
                   'srl_policy_head', 'srl_pool2x2', 'srl_qnet_build_info', 'srl_qnet_last_error', 'srl_replay_gather', 'srl_replay_scatter', 'srl_tact_bwd', 'srl_tact_bwd_blocks',
                   'srl_tact_bwd_scratch_floats', 'srl_tconv', 'srl_tcorr_grad', 'srl_td_epilogue', 'srl_tflip', 'srl_thead_bwd', 'srl_thead_fwd', 'srl_thin_conv3x3_bias_relu_f32', 'srl_thin_conv3x3_relu_project_f32', 'srl_tlayout', 'srl_train_conv_last_error', 'srl_trepack', 'srl_tu8_to_f32', 'srl_tvalue_bwd', 'srl_tvalue_fwd', 'srl_twrw', 'srl_twrw_scratch_floats', 'srl_xcorr_forward',
                   'srl_xcorr_mfma', 'srl_xcorr_mfma_last_error', 'srl_xcorr_mfma_scratch_bytes']
  L = ctypes.CDLL(build.QLIB)
  for n in names:
    assert hasattr(L, n), 'missing export ' + n


def test_qnet_signature_table_matches_the_headers():
  """`qops._SIGS` names the 67 exports the four headers declare (their types: test_header_table_and_exports_agree[qnet])."""
  from stackrl_amd import qops
  decl = boundary.declarations(boundary.ROWS['qnet'].headers)
  assert len(boundary.ROWS['qnet'].headers) == 4 and len(decl) == 67 and sorted(qops._SIGS) == sorted(decl)


def test_qnet_error_accessors_match_the_sources():
  """Every .hip file keeps its own error text: the accessor the table names for an export is the one of the file that defines
  the export (qnet.hip, greedy.hip and heuristics.hip share `srl_qnet_last_error` through `srl_qnet_set_error`)."""
  from stackrl_amd import qops
  defined = boundary.defined('qnet')
  where = {n: f for n, (f, _) in defined.items()}
  launches = {n: ret == 'int' for n, (_, ret) in defined.items()}    # status returns; the size and support queries return int32_t / int64_t
  assert len(where) == 67 and len(set(where.values())) == 9
  assert sorted(where) == sorted(qops._SIGS)
  own = {f: [n for n, g in where.items() if g == f and n.endswith('_last_error')] for f in build.QSRC}
  assert all(len(v) == 1 for f, v in own.items() if f not in ('greedy.hip', 'heuristics.hip')), own
  for f in ('greedy.hip', 'heuristics.hip'):
    with open(os.path.join(build.CSRC, f)) as fh:
      assert own[f] == [] and 'srl_qnet_set_error' in fh.read()
    own[f] = own['qnet.hip']
  assert len({v[0] for v in own.values()}) == 7
  for name, (_, _, err) in qops._SIGS.items():
    assert err == (own[where[name]][0] if launches[name] else None), name


_P = 64      # a non-null pointer: a refusal comes before anything is read through it
_CONV3X3 = ': bad arguments (H, W multiples of 16; cin in {16, 32, 64}, cout in {16, 32})'
_THIN = ': bad arguments (cin in {1, 2}; in_dtype 0 = uint8 / 255, 1 = float32)'
_THIN_CONV = ': bad arguments (H, W multiples of 16; cin in {1, 2}; in_dtype 0 = uint8 / 255, 1 = float32)'
_CONVT = ': bad arguments (W a multiple of 16; 32 -> 16 or 64 -> 32 channels)'
_GEMM = ': bad arguments (layers: srl_conv3x3_gemm_supported; the batch a multiple of srl_conv3x3_gemm_batch_multiple)'
_CONVT_GEMM = ': bad arguments (128 -> 64 or 256 -> 128 channels)'
_BIAS_ACT = ': bad arguments (channel counts, strides and offsets must be multiples of 8)'
_BIAS_BWD = ': bad arguments (C a multiple of 8 that divides 2,048, at most 256)'
_PLAIN = ': bad arguments'
# (export, arguments without the stream, the text after the export's name): one refused call per export of conv_mfma.hip,
# conv_gemm.hip and epilogue.hip that launches, and one per clause of a check that a bf16 / _f32 pair shares
_REFUSED = [
  # in, wfrag, bias, out, pooled, B, H, W, cin, cout, out_stride, out_offset, nchw
  ('srl_conv3x3_bias_relu', (None, _P, _P, _P, None, 2, 16, 16, 16, 16, 16, 0, 0), _CONV3X3),
  ('srl_conv3x3_bias_relu', (_P, _P, _P, _P, None, 2, 17, 16, 16, 16, 16, 0, 0), _CONV3X3),
  ('srl_conv3x3_bias_relu', (_P, _P, _P, _P, None, 2, 16, 16, 48, 16, 16, 0, 0), _CONV3X3),
  ('srl_conv3x3_bias_relu', (_P, _P, _P, _P, None, 2, 16, 16, 16, 16, 16, 2, 0), _CONV3X3),
  ('srl_conv3x3_bias_relu', (_P, _P, _P, _P, _P, 2, 16, 16, 16, 16, 16, 0, 1), _CONV3X3),
  ('srl_conv3x3_bias_relu_f32', (_P, _P, _P, _P, None, 2, 17, 16, 16, 16, 16, 0, 0), _CONV3X3),
  ('srl_conv3x3_bias_relu_f32', (_P, _P, _P, _P, _P, 2, 16, 16, 64, 32, 32, 0, 1), _CONV3X3),
  # in, in_dtype, w, bias, out, B, H, W, cin, Hp, Wp
  ('srl_conv3x3_thin', (_P, 0, _P, _P, _P, 2, 16, 16, 3, 16, 16), _THIN),
  ('srl_conv3x3_thin', (_P, 2, _P, _P, _P, 2, 16, 16, 1, 16, 16), _THIN),
  ('srl_conv3x3_thin', (_P, 0, _P, _P, _P, 2, 16, 16, 1, 15, 16), _THIN),
  ('srl_conv3x3_thin_f32', (_P, 1, _P, _P, None, 2, 16, 16, 2, 16, 16), _THIN),
  # in, wfrag, bias, proj_w, proj_b, out, B, H, W, Hv, Wv
  ('srl_conv3x3_relu_project', (_P, _P, _P, _P, 0.5, _P, 2, 17, 16, 16, 16), _PLAIN),
  ('srl_conv3x3_relu_project', (_P, _P, _P, _P, 0.5, _P, 2, 16, 16, 17, 16), _PLAIN),
  ('srl_conv3x3_relu_project', (_P, _P, _P, None, 0.5, _P, 2, 16, 16, 16, 16), _PLAIN),
  ('srl_conv3x3_relu_project_f32', (_P, _P, _P, _P, 0.5, _P, 2, 32, 32, 20, 0), _PLAIN),
  # in, in_dtype, cin, w1, b1, wfrag, bias, out, pooled, B, H, W, out_stride, out_offset, nchw
  ('srl_thin_conv3x3_bias_relu_f32', (_P, 0, 3, _P, _P, _P, _P, _P, None, 2, 16, 16, 16, 0, 0), _THIN_CONV),
  ('srl_thin_conv3x3_bias_relu_f32', (_P, 0, 1, _P, _P, _P, _P, _P, _P, 2, 16, 16, 16, 0, 1), _THIN_CONV),
  # in, w1, b1, wfrag, bias, proj_w, proj_b, out, B, H, W
  ('srl_thin_conv3x3_relu_project_f32', (_P, _P, None, _P, _P, _P, 0.5, _P, 2, 20, 20), _PLAIN),
  ('srl_thin_conv3x3_relu_project_f32', (_P, _P, _P, _P, _P, _P, 0.5, _P, 2, 0, 20), _PLAIN),
  # in, wfrag, bias, out, B, H, W, cin, cout, out_stride, out_offset
  ('srl_convt2x2_bias_relu', (_P, _P, _P, _P, 2, 8, 24, 32, 16, 32, 0), _CONVT),
  ('srl_convt2x2_bias_relu', (_P, _P, _P, _P, 2, 8, 16, 32, 32, 32, 0), _CONVT),
  ('srl_convt2x2_bias_relu', (_P, _P, _P, _P, 2, 8, 16, 32, 16, 32, 2), _CONVT),
  ('srl_convt2x2_bias_relu_f32', (_P, _P, _P, _P, 2, 8, 16, 128, 64, 128, 0), _CONVT),
  # in, wfrag, bias, out, B, W, cin, cout, out_stride, out_offset, f32
  ('srl_conv3x3_gemm_bias_relu', (_P, _P, _P, _P, 2, 32, 16, 64, 64, 0, 0), _GEMM),
  ('srl_conv3x3_gemm_bias_relu', (_P, _P, _P, _P, 3, 8, 128, 256, 256, 0, 1), _GEMM),
  ('srl_conv3x3_gemm_bias_relu', (_P, None, _P, _P, 2, 32, 32, 64, 64, 0, 1), _GEMM),
  # in, wfrag, bias, out, B, H, W, cin, cout, out_stride, out_offset, f32
  ('srl_convt2x2_gemm_bias_relu', (_P, _P, _P, _P, 2, 8, 8, 64, 32, 64, 0, 0), _CONVT_GEMM),
  ('srl_convt2x2_gemm_bias_relu', (_P, _P, _P, _P, 2, 8, 8, 128, 64, 128, 2, 1), _CONVT_GEMM),
  # in, out, bias, npix, C, out_stride, out_offset, nchw_hw, relu
  ('srl_bias_act', (_P, _P, _P, 10, 12, 16, 0, 0, 1), _BIAS_ACT),
  ('srl_bias_act', (_P, _P, _P, 10, 16, 16, 2, 0, 1), _BIAS_ACT),
  ('srl_bias_act', (_P, _P, _P, 10, 16, 16, 0, 3, 1), _BIAS_ACT),
  ('srl_bias_act_f32', (_P, _P, None, 10, 16, 16, 0, 0, 1), _BIAS_ACT),
  # in, skip, pooled, bias, B, H, W, C, skip_stride, skip_offset
  ('srl_bias_act_pool', (_P, _P, _P, _P, 2, 3, 4, 16, 16, 0), _PLAIN),
  ('srl_bias_act_pool', (_P, _P, _P, _P, 2, 4, 4, 12, 16, 0), _PLAIN),
  ('srl_bias_act_pool', (_P, _P, _P, _P, 2, 4, 4, 16, 20, 0), _PLAIN),
  ('srl_bias_act_pool_f32', (_P, _P, None, _P, 2, 4, 4, 16, 16, 0), _PLAIN),
  # gy, y, gx, gbias, scratch, npix, C, relu
  ('srl_bias_act_bwd_f32', (_P, _P, _P, _P, _P, 10, 12, 1), _BIAS_BWD),
  ('srl_bias_act_bwd_f32', (_P, None, _P, _P, _P, 10, 16, 1), _BIAS_BWD),
  # in, pooled, B, H, W, C, in_stride, in_offset, f32
  ('srl_pool2x2', (_P, _P, 2, 3, 4, 16, 16, 0, 0), _PLAIN),
  ('srl_pool2x2', (_P, _P, 2, 4, 4, 16, 16, 4, 1), _PLAIN),
]


def test_rollout_conv_exports_refuse_bad_arguments_with_their_own_text():
  """Every launching export of conv_mfma.hip, conv_gemm.hip and epilogue.hip returns 1 for arguments it refuses (before any
  HIP call: no GPU needed) and leaves "<its own name>: bad arguments..." behind its file's accessor."""
  from stackrl_amd import build, qops
  build.build()
  L = ctypes.CDLL(build.QLIB)
  files = {qops._CONV: 'conv_mfma.hip', qops._GEMM: 'conv_gemm.hip', qops._EPI: 'epilogue.hip'}
  launching = {n for n, (res, _, err) in qops._SIGS.items() if err in files}
  assert {n for n, _, _ in _REFUSED} == launching and len(launching) == 18
  for name, args, tail in _REFUSED:
    res, argtypes, err = qops._SIGS[name]
    f = getattr(L, name)
    f.restype, f.argtypes = res, argtypes
    last = getattr(L, err)
    last.restype, last.argtypes = ctypes.c_char_p, []
    assert len(args) + 1 == len(argtypes), name
    assert f(*args, None) == 1, (name, args)
    assert last().decode() == name + tail, (name, args)


_X_PLAIN = 'srl_xcorr_mfma: bad arguments'
_X_SHAPE = 'srl_xcorr_mfma: unsupported mode %d / shape %d, %d (128 / 32 and 64 / 16 are built)'
_X_ROWS = 'srl_xcorr_rows: bad arguments (128 / 32 maps of at most 16 channels; bf16x3 needs float32 operands)'
_X_BIG = 1 << 40      # scratch_bytes that any shape fits
# (export, arguments without the stream, the whole text): one refused call per clause of the two checks of xcorr_mfma.hip
_XCORR_REFUSED = [
  # mode, precision, in, in_f32, kern, kern_f32, out, scratch, scratch_bytes, B, C, H, kh
  ('srl_xcorr_mfma', (0, 0, None, 1, _P, 1, _P, _P, _X_BIG, 3, 16, 128, 32), _X_PLAIN),
  ('srl_xcorr_mfma', (0, 0, _P, 1, _P, 1, _P, _P, _X_BIG, 0, 16, 128, 32), _X_PLAIN),
  ('srl_xcorr_mfma', (0, 2, _P, 1, _P, 1, _P, _P, _X_BIG, 3, 16, 128, 32), _X_PLAIN),
  ('srl_xcorr_mfma', (0, 0, _P, 1, _P, 1, _P, None, _X_BIG, 3, 16, 128, 32), _X_PLAIN),      # 3 samples of 16 channels: partials
  ('srl_xcorr_mfma', (0, 0, _P, 1, _P, 1, _P, _P, _X_BIG, 3, 16, 100, 32), _X_SHAPE % (0, 100, 32)),
  ('srl_xcorr_mfma', (3, 0, _P, 1, _P, 1, _P, _P, _X_BIG, 3, 16, 128, 32), _X_SHAPE % (3, 128, 32)),
  ('srl_xcorr_mfma', (0, 0, _P, 1, _P, 1, _P, _P, 1024, 3, 16, 128, 32), 'srl_xcorr_mfma: scratch too small'),
  ('srl_xcorr_mfma', (0, 1, _P, 0, _P, 1, _P, _P, _X_BIG, 3, 16, 128, 32),
   'srl_xcorr_mfma: precision 1 (bf16x3) takes float32 operands'),
  # precision, in, kern, f32, out, B, C, H, kh
  ('srl_xcorr_rows', (0, _P, _P, 1, _P, 3, 17, 128, 32), _X_ROWS),
  ('srl_xcorr_rows', (0, _P, _P, 1, _P, 3, 16, 64, 32), _X_ROWS),
  ('srl_xcorr_rows', (1, _P, _P, 0, _P, 3, 16, 128, 32), _X_ROWS),
  ('srl_xcorr_rows', (0, _P, _P, 1, None, 3, 16, 128, 32), _X_ROWS),
]


def test_xcorr_exports_refuse_bad_arguments_with_their_own_text():
  """`srl_xcorr_mfma` and `srl_xcorr_rows` return 1 for arguments they refuse (before any HIP call: no GPU needed) and leave
  their text behind `srl_xcorr_mfma_last_error`: one call per clause of their checks."""
  from stackrl_amd import build, qops
  build.build()
  L = ctypes.CDLL(build.QLIB)
  launching = {n for n, (res, _, err) in qops._SIGS.items() if err == qops._XCORR}
  assert {n for n, _, _ in _XCORR_REFUSED} == launching and len(launching) == 2
  last = L.srl_xcorr_mfma_last_error
  last.restype, last.argtypes = ctypes.c_char_p, []
  for name, args, text in _XCORR_REFUSED:
    res, argtypes, _ = qops._SIGS[name]
    f = getattr(L, name)
    f.restype, f.argtypes = res, argtypes
    assert len(args) + 1 == len(argtypes), name
    assert f(*args, None) == 1, (name, args)
    assert last().decode() == text, (name, args)


def test_config_struct_matches_header():
  from stackrl_amd.config import CConfig, StackConfig
  with open(os.path.join(ROOT, 'include', 'srl_types.h')) as f:
    txt = f.read()
  body = txt[txt.index('typedef struct srl_config {'):txt.index('} srl_config;')]
  fields = re.findall(r'^\s*(?:int32_t|float)\s+([a-z_]+);', body, re.M)
  assert fields == [f[0] for f in CConfig._fields_]
  L = ctypes.CDLL(__import__('stackrl_amd.build', fromlist=['x']).build())
  c = CConfig()
  assert L.srl_config_default(ctypes.byref(c)) == 0
  d = StackConfig(episode_length=30).to_c()
  for name, _ in CConfig._fields_:
    if name == 'max_substeps':     # 0 = "derive it" in the C default; the host mirror hands over int(300 / time_step) (simulator.py:46)
      assert c.max_substeps == 0 and d.max_substeps == 30000
      continue
    assert getattr(c, name) == pytest.approx(getattr(d, name)), name


def test_config_validation_mirrors_reference_errors():
  from stackrl_amd.config import StackConfig
  with pytest.raises(ValueError, match='Invalid value .* for argument dtype'):   # env.py:169-170
    StackConfig(dtype='float33')
  with pytest.raises(ValueError):
    StackConfig(reward_params=-1)                                                # rewarder.py:132-133
  assert StackConfig(rewarder='position').metric_id == 3                          # env.py:148-151
  assert StackConfig(rewarder='occupation').metric_id == 1
  assert StackConfig(rewarder=None).metric_id == 0                                # rewarder.py:113-114
  c = StackConfig.config_gin(episode_length=8).to_c()
  assert c.sim_time_step == pytest.approx(0.0125) and c.metric == 3 and c.reward_scale < 0
  assert StackConfig(resolution_factor=4).n_actions == 2401


def test_product_has_no_oracle_dependency():
  """The product package must not import, include, link or call anything under oracle/."""
  pkg = os.path.join(ROOT, 'stackrl_amd')
  bad = re.compile(r'(import\s+oracle|from\s+oracle|oracle/|oracle\.py|srlo_|libsrl_oracle|srl_oracle)')
  for dirpath, _, files in os.walk(pkg):
    for f in files:
      if f.endswith(('.py', '.hip', '.h')):
        with open(os.path.join(dirpath, f)) as fh:
          src = fh.read()
        assert not bad.search(src), os.path.join(dirpath, f)


def test_env_requires_gpu_loudly():
  torch = pytest.importorskip('torch')
  if torch.cuda.is_available():
    pytest.skip('GPU present')
  from stackrl_amd import env
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    env.VecStackEnv(n_parallel=2)
