"""The GPU suite reaches every layer path of the product's rollout forward (no GPU needed).

`qops.FastFeatures` routes every layer of the two U-Nets by map size, dtype mode and batch (tests/rollout_dispatch.py restates
the routing and names a PATH per layer).  A kernel compared with a reference only at the Stack-v0 shape and at one batch is
compared on other paths than the product runs: at 64 x 64 observations (BASELINE configs[4]) the left U-Net uses five
instantiations of `k_conv3x3_gemm` of its own and the right U-Net's 8^2 and 4^2 levels fall to library convolutions plus the
passes of csrc/epilogue.hip; at a batch that is no multiple of 8 the layers whose workgroups take eight maps fall to the
library too; and at 8 samples those layers run as ONE workgroup, so the kernel's map offset is never anything but 0.

This module
  * holds the restatement to the library's exports (host arithmetic, no GPU call) for every (cin, cout, W) in
    {16 .. 256}^2 x {4, 8, 16, 32}, and the list of gemm layers to the `SRL_CASE` lines of csrc/conv_gemm.hip, so that an
    instantiation added later without a test case fails here;
  * enumerates the paths of the product's rollout (`product_rollout_regimes`) and the paths the parameter lists of the GPU
    tests reach — imported from the GPU test modules, so that the two cannot drift apart — and asserts that the second set
    contains the first."""
import ctypes
import os
import re

import pytest

import rollout_dispatch as D

torch = pytest.importorskip('torch')        # the GPU test modules import it at their top

import test_learner_gpu as TL               # noqa: E402  (parameter lists only; nothing in them runs at import)
import test_rollout_forward_gpu as TR       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_GEMM_SOURCE = os.path.join(ROOT, 'stackrl_amd', 'csrc', 'conv_gemm.hip')
PRECISIONS = ('bf16', 'bf16x3')


def srl_cases(path=CONV_GEMM_SOURCE):
  """(cin, cout, W) of every `SRL_CASE(ci, co, w)` line of the source text (the macro's own definition has no numbers)."""
  with open(path) as f:
    return [tuple(int(v) for v in m) for m in re.findall(r'SRL_CASE\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)', f.read())]


def gemm_case_regimes(layers, batch=None):
  """test_conv3x3_gemm_matches_torch_fp64 ((cin, cout, W) at `batch` samples) or
  test_conv3x3_gemm_past_the_first_workgroup ((cin, cout, W, B)), both precisions."""
  return {D.gemm_regime(c[0], c[1], c[2], p, batch if batch is not None else c[3]) for c in layers for p in PRECISIONS}


def epilogue_case_regimes(kernel, dtypes, forms, channels, maps, relus, batch):
  paths, launches = set(), set()
  for dt in dtypes:
    for form in forms:
      for C in channels:
        for H, W in maps:
          for relu in relus:
            path, launch = D.epilogue_regime(kernel, dt, form, batch * H * W, C, relu)
            paths.add(path); launches.add((kernel,) + launch)
  return paths, launches


def forward_case_regimes(cases):
  out = set()
  for (res_l, res_r), mode, B in cases:
    out |= set(D.forward_paths(res_l, res_r, mode, B))
    out.add(D.forward_regime(res_l, res_r, mode, B))
  return out


def regimes_reached(gemm8=None, gemm2m=None, epilogues=True, forward=None, independence=None, policy=None):
  """The paths the GPU suite reaches with the given parameter lists (default: the lists of the GPU test modules)."""
  out = gemm_case_regimes(TL._GEMM_LAYERS if gemm8 is None else gemm8, TL._GEMM_BATCH)
  out |= gemm_case_regimes(TR.GEMM_TWO_GROUP_CASES if gemm2m is None else gemm2m)
  if epilogues:
    out |= epilogue_case_regimes('bias_act', TR.EPILOGUE_DTYPES, TR.BIAS_ACT_FORMS, TR.EPILOGUE_CHANNELS, TR.BIAS_ACT_MAPS, (True, False),
                                 TR.EPILOGUE_BATCH)[0]
    out |= epilogue_case_regimes('bias_act_pool', TR.EPILOGUE_DTYPES, ('slice+pool',), TR.EPILOGUE_CHANNELS, TR.POOL_MAPS, (True,),
                                 TR.EPILOGUE_BATCH)[0]
  out |= forward_case_regimes(TR.FORWARD_CASES if forward is None else forward)
  # the other two tests of the forward compare it with itself, or its actions with float64: they reach their layers' paths,
  # but they are no comparison of a whole forward with a reference
  for shape, mode in TR.INDEPENDENCE_CASES if independence is None else independence:
    assert TR.INDEPENDENCE_BATCH == 16
    out |= {r for r in forward_case_regimes([(shape, mode, 16), (shape, mode, 8)]) if r[0] != 'forward'}
    out.add(D.forward_check('position independence', shape, mode))
  for shape, mode in TR.POLICY_CASES if policy is None else policy:
    assert (TR.POLICY_BATCH, TR.POLICY_CHUNKS) == (20, (8, 32))
    for chunk in TR.POLICY_CHUNKS:
      out |= {r for r in forward_case_regimes([(shape, mode, b) for b in D.policy_chunks(20, chunk)]) if r[0] != 'forward'}
    out.add(D.forward_check('policy chunks', shape, mode))
  return out


# The lists of the GPU tests before this module existed: 13 gemm layers at 8 samples, and the forward compared with a reference
# at 128 / 32 and 6 samples only (test_fast_features_match_autocast_features, test_fast_features_fp32_match_the_module;
# test_fast_rollout_with_and_without_the_fused_first_level runs 8 samples but compares two runs of the same kernels)
EARLIER_LISTS = dict(
  gemm8=[(32, 64, 32), (64, 64, 32), (128, 64, 32), (64, 128, 16), (128, 128, 16), (256, 128, 16), (128, 256, 8), (256, 256, 8),
         (32, 64, 8), (64, 64, 16), (128, 64, 16), (256, 128, 8), (128, 256, 4)],
  gemm2m=[], epilogues=False, forward=[((128, 32), 'bf16', 6), ((128, 32), 'fp32-class', 6), ((128, 32), 'fp32 epilogues only', 6)],
  independence=[], policy=[])


def _show(regimes):
  return '\n'.join('  ' + ' '.join(str(v) for v in r) for r in sorted(regimes, key=str))


def test_the_gpu_suite_reaches_every_path_of_the_rollout():
  need = D.product_rollout_regimes() | D.product_forward_checks()
  missing = need - regimes_reached()
  assert not missing, 'paths of the rollout forward that no GPU test reaches:\n' + _show(missing)
  # the gemm instantiations and the epilogue passes by the tests of the single kernels alone: the whole forward's test says
  # that a feature is off, theirs say which kernel's
  single = {r for r in need if r[0] in ('conv_gemm', 'library+bias_act', 'library+bias_act_pool')}
  missing = single - regimes_reached(forward=[], independence=[], policy=[])
  assert not missing, 'kernel paths of the rollout that only the whole forward\'s test reaches:\n' + _show(missing)


def test_every_gemm_instantiation_has_its_cases():
  """`SRL_CASE` lines == the restatement's supported layers == the layers of both GPU lists; the second list runs each layer at
  twice its batch multiple (the smallest launch in which a workgroup starts past the first map)."""
  src = srl_cases()
  assert len(src) == len(set(src)) == 18
  assert set(src) == set(D.gemm_layers())
  for name, layers in (('_GEMM_LAYERS', TL._GEMM_LAYERS), ('GEMM_TWO_GROUP_CASES', [c[:3] for c in TR.GEMM_TWO_GROUP_CASES])):
    assert len(layers) == len(set(layers)), name
    missing, extra = set(src) - set(layers), set(layers) - set(src)
    assert not missing and not extra, '{}: instantiations without a case {}, cases without an instantiation {}'.format(
      name, sorted(missing), sorted(extra))
  for cin, cout, W, B in TR.GEMM_TWO_GROUP_CASES:
    assert B == 2 * D.conv3x3_gemm_batch_multiple(cout, W), (cin, cout, W, B)
    assert D.gemm_first_maps(cout, W, B) == [0, B // 2], (cin, cout, W, B)
  assert TL._GEMM_BATCH == 8
  assert sorted({c[3] for c in TR.GEMM_TWO_GROUP_CASES}) == [2, 4, 8, 16]


def test_an_instantiation_added_without_a_case_is_noticed(tmp_path):
  with open(CONV_GEMM_SOURCE) as f:
    text = f.read()
  p = tmp_path / 'conv_gemm.hip'
  p.write_text(text.replace('#undef SRL_CASE', '  SRL_CASE(256, 128, 4)\n#undef SRL_CASE', 1))
  assert set(srl_cases(str(p))) - set(TL._GEMM_LAYERS) == {(256, 128, 4)}


def test_the_epilogue_cases_reach_every_launch_shape():
  """One block and several, a full last block and a partial one, for both kernels (the element counts of the issue's shapes)."""
  # the cases the kernels are held to, on record: both dtypes; in place, a slice of a wider buffer, NCHW (which only the
  # epilogues-only mode of the forward uses: no product path asks for it); one thread per pixel (8 channels) and several;
  # maps whose pooled width is even and odd, and an odd map for the pass without the pool
  assert set(TR.EPILOGUE_DTYPES) == {'bf16', 'f32'} and set(TR.BIAS_ACT_FORMS) == {'in place', 'slice', 'nchw'}
  assert set(TR.EPILOGUE_CHANNELS) == {8, 32, 64} and set(TR.POOL_MAPS) == {(8, 8), (4, 6)} and TR.EPILOGUE_BATCH == 3
  assert set(TR.BIAS_ACT_MAPS) == {(8, 8), (4, 6), (5, 7)}
  _, launches = epilogue_case_regimes('bias_act', TR.EPILOGUE_DTYPES, TR.BIAS_ACT_FORMS, TR.EPILOGUE_CHANNELS, TR.BIAS_ACT_MAPS, (True, False),
                                      TR.EPILOGUE_BATCH)
  for relu in ('relu', 'no relu'):
    for shape in (('one block', 'partial last block'), ('more blocks', 'partial last block'), ('more blocks', 'full last block')):
      assert ('bias_act', relu) + shape in launches
  _, launches = epilogue_case_regimes('bias_act_pool', TR.EPILOGUE_DTYPES, ('slice+pool',), TR.EPILOGUE_CHANNELS, TR.POOL_MAPS, (True,),
                                      TR.EPILOGUE_BATCH)
  for shape in (('one block', 'partial last block'), ('more blocks', 'partial last block')):
    assert ('bias_act_pool', 'relu') + shape in launches


def test_the_product_reaches_what_the_earlier_lists_never_did():
  """The reason for the added cases, kept as a test: with the earlier lists these paths of the product had no numeric test."""
  missing = D.product_rollout_regimes() - regimes_reached(**EARLIER_LISTS)
  print(_show(missing))
  for prec in PRECISIONS:
    for layer in ((64, 64, 8), (32, 64, 16), (64, 128, 8), (128, 128, 8), (256, 256, 4)):    # never run at all
      assert ('conv_gemm',) + layer + (prec, 'multi-wg') in missing
    for layer in ((32, 64, 8), (128, 256, 4)):      # run, but as one workgroup: `img0` only ever 0
      assert ('conv_gemm',) + layer + (prec, 'multi-wg') in missing
    assert ('conv_gemm', 32, 64, 32, prec, 'multi-wg') not in missing
  assert ('library+bias_act_pool', 'f32') not in missing         # (the epilogues-only forward ran it, inside a whole-network comparison)
  for r in [('library+bias_act_pool', 'bf16'), ('tconv 1x1 d2s', 32, 16),
            ('forward', '64/16', 'bf16', 'batch multiple of 8'), ('forward', '64/16', 'fp32-class', 'batch multiple of 1'),
            ('forward', '128/32', 'bf16', 'batch multiple of 8'), ('forward', '128/32', 'fp32-class', 'batch multiple of 1')]:
    assert r in missing, r


def test_the_hand_worked_routes_of_the_rollout():
  """The routing at the product's shapes, worked by hand from `FastFeatures._unet` (a wrong restatement would move these)."""
  assert D.product_batches((128, 32)) == [1024, 2048, 7] and D.product_batches((64, 16)) == [1024, 7]
  assert D.policy_chunks(20, 8) == [8, 8, 4] and D.policy_chunks(20, 32) == [20] and D.batch_class(20) == 4
  c = D.gemm_cfg(64, 32, True)
  assert (c['NI'], c['PARTS'], c['RT'], c['SWZ']) == (1, 2, 16, True) and not D.gemm_cfg(64, 32)['SWZ'] and not D.gemm_cfg(64, 16, True)['SWZ']
  assert [D.conv3x3_gemm_batch_multiple(co, w) for co, w in ((64, 32), (64, 16), (64, 8), (128, 16), (128, 8), (256, 8), (256, 4))] == \
    [1, 2, 8, 1, 4, 2, 8]
  assert D.gemm_workgroups(64, 32, 8) == 16 and D.gemm_workgroups(64, 8, 8) == 1 and D.gemm_workgroups(256, 4, 16) == 2
  # 128 / 32, eight samples, fp32-class: no library call at all; bf16: the right U-Net's 64 -> 32 transposed convolution at 8 x 8
  p = D.forward_paths(128, 32, 'fp32-class', 8)
  assert not D.has_library_call(p) and len(p) == 23 + 11 + 1      # left: 26 layers, the fused first level one call, two pools; right: 12 layers; the head
  assert p[0] == ('thin+conv fused', 2, 'uint8', 'slice+pool') and p[-1] == ('pos fused',)
  assert ('conv_gemm', 64, 64, 8, 'bf16x3', 'one-wg') in p and ('tconv 1x1 d2s', 64, 32) in p
  p = D.forward_paths(128, 32, 'bf16', 8)
  assert [q for q in p if q[0].startswith('library')] == [('library+bias_act', 'bf16', 'slice')]
  # ... and at seven samples every layer with a batch multiple above 1 is the library's
  p = D.forward_paths(128, 32, 'bf16', 7)
  assert {q[1:4] for q in p if q[0] == 'conv_gemm'} == {(32, 64, 32), (64, 64, 32), (128, 64, 32), (64, 128, 16), (128, 128, 16), (256, 128, 16)}
  assert p.count(('library+bias_act', 'bf16', 'in place')) == 4
  # 64 / 16, bf16: the right U-Net's 8^2 level and 4^2 bottom are library convolutions, its two transposed convolutions too
  right = D._unet_paths(16, 1, 2, 'bf16', 1024)
  assert right == [('thin', 1, 'uint8', 'bf16'), ('conv_mfma', 16, 16, 'slice+pool', 'bf16'),
                   ('library+bias_act', 'bf16', 'in place'), ('library+bias_act_pool', 'bf16'),
                   ('library+bias_act', 'bf16', 'in place'), ('library+bias_act', 'bf16', 'in place'),
                   ('library+bias_act', 'bf16', 'slice'), ('library+bias_act', 'bf16', 'in place'), ('library+bias_act', 'bf16', 'in place'),
                   ('library+bias_act', 'bf16', 'slice'), ('conv_mfma', 32, 16, 'plain', 'bf16'), ('conv_mfma', 16, 16, 'nchw', 'bf16')]
  left = D._unet_paths(64, 2, 4, 'bf16', 1024)
  assert [q[1:4] for q in left if q[0] == 'conv_gemm'] == [(32, 64, 16), (64, 64, 16), (64, 128, 8), (128, 128, 8), (128, 256, 4), (256, 256, 4),
                                                          (256, 128, 8), (128, 128, 8), (128, 64, 16), (64, 64, 16)]
  # the transposed form of the epilogue (`nchw`) is reached by no hand-written mode of the product: both U-Nets end on
  # csrc/conv_mfma.hip's own NCHW store (maps of 128, 64, 32 and 16 pixels are whole tiles); only the epilogues-only mode uses it
  assert not any(q[0] == 'library+bias_act' and q[2] == 'nchw' for q in D.product_rollout_regimes())
  assert D.forward_paths(64, 16, 'fp32 epilogues only', 8).count(('library+bias_act', 'f32', 'nchw')) == 2


def test_the_restatement_is_the_library_s_arithmetic():
  from stackrl_amd import build
  build.build()
  L = ctypes.CDLL(build.QLIB)       # host-side arithmetic only: no GPU call
  I32, I64 = ctypes.c_int32, ctypes.c_int64
  for name, res, nargs in (('srl_conv3x3_gemm_supported', I32, 3), ('srl_conv3x3_gemm_batch_multiple', I32, 2),
                           ('srl_conv3x3_gemm_wfrag_elems', I64, 2), ('srl_convt2x2_gemm_supported', I32, 2),
                           ('srl_conv3x3_wfrag_elems', I32, 2), ('srl_convt2x2_wfrag_elems', I32, 2)):
    getattr(L, name).restype = res
    getattr(L, name).argtypes = [I32] * nargs
  chans = (16, 32, 64, 128, 256)
  supported = set()
  for cin in chans:
    for cout in chans:
      assert L.srl_conv3x3_gemm_wfrag_elems(cin, cout) == D.conv3x3_gemm_wfrag_elems(cin, cout), (cin, cout)
      assert bool(L.srl_convt2x2_gemm_supported(cin, cout)) == D.convt2x2_gemm_supported(cin, cout), (cin, cout)
      assert L.srl_conv3x3_wfrag_elems(cin, cout) == D.conv3x3_wfrag_elems(cin, cout), (cin, cout)
      assert L.srl_convt2x2_wfrag_elems(cin, cout) == D.convt2x2_wfrag_elems(cin, cout), (cin, cout)
      for W in (4, 8, 16, 32):
        assert bool(L.srl_conv3x3_gemm_supported(cin, cout, W)) == D.conv3x3_gemm_supported(cin, cout, W), (cin, cout, W)
        if D.conv3x3_gemm_supported(cin, cout, W):
          supported.add((cin, cout, W))
          assert L.srl_conv3x3_gemm_batch_multiple(cout, W) == D.conv3x3_gemm_batch_multiple(cout, W), (cout, W)
  assert supported == set(D.gemm_layers()) == set(srl_cases())
