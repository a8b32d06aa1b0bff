"""The GPU suite reaches every host-side dispatch regime of the product's update (no GPU needed).

The update the product and the benchmark run is `minibatch_size=32` with Double-DQN: `HandNet.forward` sees 64 samples, the
target net 32, `HandNet.backward` the first 32.  The host side of the kernels behind it picks template instantiations and loop
structures from the batch size (tests/update_dispatch.py restates those choices and names a REGIME per launch), so a kernel
compared with a reference at 1 - 6 samples only is compared in other code paths than the product runs: `k_tconv` with one
output-channel tile per workgroup instead of 2 or 4, `k_twrw` with one pixel tile per group and no group without one,
`k_tact_bwd` at its minimal block, `k_xcorr_mfma` with one channel per workgroup (no prefetch of the next channel, no
accumulator reset between channels).

This module
  * holds the restatement to the library where the library exports the quantity (`srl_twrw_scratch_floats`,
    `srl_tact_bwd_blocks`, `srl_xcorr_mfma_scratch_bytes`: host arithmetic, no GPU call); `launch_conv`'s choice of output
    channels per workgroup has no export: profiles/update_batch_tests_kernel_names.txt is the kernel-name summary of a
    traced run of the update-path GPU tests, with k_tconv at COT 1, 2 and 4 for both tap counts;
  * enumerates the regimes of the product's update (every layer of `DeepQSiamFCN` for the Stack-v0 shapes and the 64 x 64
    configuration, the three cross-correlation modes in both precisions and with the operand pairs float32 and bf16 features
    give them, the rollout's forward at a policy chunk of 256 samples) and the regimes the parameter lists of the GPU
    tests reach — imported from the GPU test modules, so that the two cannot drift apart — and asserts that the second set
    contains the first, and the ragged channel splits besides."""
import ctypes

import pytest

import update_dispatch as D

torch = pytest.importorskip('torch')        # the GPU test modules import it at their top

import test_learner_gpu as TL               # noqa: E402  (parameter lists only; nothing in them runs at import)
import test_train_conv_gpu as TC            # noqa: E402
import test_xcorr_exact_gpu as TX           # noqa: E402


def conv_case_regimes(cin, cout, B, H, W):
  """test_conv3x3_forward_data_and_weight_gradients_match_torch_fp64: forward, activation gradient, weight gradient, data
  gradient to the input channels padded to 16."""
  return {D.tconv_regime(9, B, H, W, cout), D.tact_regime(B, H, W, cout), D.twrw_regime(9, B, H, W, cin, cout),
          D.tconv_regime(9, B, H, W, (cin + 15) // 16 * 16)}


def convt_case_regimes(cin, cout, B, H, W):
  """test_transposed_conv_forward_and_gradients_match_torch_fp64: the 1 x 1 form to 4 cout channels on the INPUT map."""
  return {D.tconv_regime(1, B, H, W, 4 * cout), D.tact_regime(B, 2 * H, 2 * W, cout, s2d=True),
          D.twrw_regime(1, B, H, W, cin, 4 * cout), D.tconv_regime(1, B, H, W, cin)}


def act_case_regimes(C, B, H, W, form):
  return {D.tact_regime(B, H, W, C, s2d=form == 's2d', pool=form == 'pool')}


def hand_net_case_regimes(rf, B, n):
  h = 2 ** rf
  out = set()
  for l in D.net_layers(4 * h, h):
    out |= D.layer_regimes(l, B, n)
  out.add(D.xcorr_regime(0, 1, B, 16, 4 * h, h))             # `HandNet`'s default precision: bf16x3
  out |= {D.xcorr_regime(m, 1, n, 16, 4 * h, h) for m in (1, 2)}
  return out


def xcorr_case_regimes(B, C, H, h, precision, force=None):
  return {D.xcorr_regime(m, precision, B, C, H, h, force=force) for m in (0, 1, 2)}


ROWS_KIND = {'f32x3': (1, (D.F32, D.F32)), 'f32': (0, (D.F32, D.F32)), 'bf16': (0, (D.BF16, D.BF16))}


def xcorr_exact_regimes():
  """tests/test_xcorr_exact_gpu.py, from its parameter lists: the Toeplitz kernel forced (SRL_XCORR_ROWS=0) in three modes with
  every operand pair at precision 0 and with the split, the forward at 256 samples, the row-product kernel forced at 3 samples
  and chosen at 192, and the autograd function under bf16 features."""
  out = set()
  for H, h in TX.GEOMETRIES:
    for B, C in TX.TOEPLITZ_BC:
      out |= {D.xcorr_regime(m, 0, B, C, H, h, (D.F32 if a == 'f32' else D.BF16, D.F32 if k == 'f32' else D.BF16), force='0')
              for m in (0, 1, 2) for a, k in TX.PAIRS}
    for B, C in TX.SPLIT_BC:
      out |= xcorr_case_regimes(B, C, H, h, 1, force='0')
    for kind in TX.ROWS_KINDS:
      precision, pair = ROWS_KIND[kind]
      out.add(D.xcorr_regime(0, precision, TX.LARGE_BATCH, 16, H, h, pair, force='0'))
    pairs = D.backward_pairs(D.BF16)
    out |= {D.xcorr_regime(m, 0, 3, 16, H, h, pairs[m], force='0') for m in (0, 1, 2)}
  for kind in TX.ROWS_KINDS:
    precision, pair = ROWS_KIND[kind]
    out |= {D.xcorr_regime(0, precision, 3, C, 128, 32, pair, force='1') for C in TX.ROWS_CHANNELS}
    out.add(D.xcorr_regime(0, precision, TX.ROWS_BATCH, 16, 128, 32, pair))
  return out


def regimes_reached(conv=None, convt=None, act=None, hand=None, xc_auto=None, xc_update=None, xc_exact=True):
  """The regimes the GPU suite reaches with the given parameter lists (default: the lists of the GPU test modules)."""
  out = xcorr_exact_regimes() if xc_exact else set()
  for c in TC.CONV3X3_CASES if conv is None else conv:
    out |= conv_case_regimes(*c)
  for c in TC.CONVT_CASES if convt is None else convt:
    out |= convt_case_regimes(*c)
  for c in TC.ACT_CASES if act is None else act:
    out |= act_case_regimes(*c)
  for c in TC.HAND_NET_CASES if hand is None else hand:
    out |= hand_net_case_regimes(*c)
  for precision, _ in TL.XCORR_PRECISIONS:
    for c in TL.XCORR_AUTOGRAD_CASES if xc_auto is None else xc_auto:
      out |= xcorr_case_regimes(*c, precision=precision)
    for c in TL.XCORR_UPDATE_CASES if xc_update is None else xc_update:
      out |= xcorr_case_regimes(*c, precision=precision, force='0')       # that test sets SRL_XCORR_ROWS=0
  for B, C, dt in TL.XCORR_ROWS_CASES:      # test_xcorr_row_product_forward: forced for small batches, then the Toeplitz kernel forced
    precision, pair = ROWS_KIND[dt]
    out.add(D.xcorr_regime(0, precision, B, C, 128, 32, pair, force=None if B >= 192 else '1'))
    out.add(D.xcorr_regime(0, precision, B, C, 128, 32, pair, force='0'))
  return out


# The lists of the GPU tests before the cases at the update's batch sizes were added (every batch 1 - 6; the whole net at 5 / 3)
SMALL_BATCH_LISTS = dict(
  conv=[(2, 16, 2, 32, 48), (1, 16, 3, 97, 97), (16, 16, 2, 48, 32), (32, 64, 5, 16, 16), (64, 32, 6, 8, 8), (128, 64, 3, 4, 4),
        (256, 256, 4, 8, 8), (48, 16, 1, 20, 17)],
  convt=[(32, 16, 2, 24, 16), (64, 32, 3, 8, 8), (256, 128, 4, 8, 8), (128, 64, 2, 5, 7)],
  act=[(16, 2, 16, 24, 'pool'), (64, 3, 8, 8, 'pool'), (256, 2, 4, 4, 'pool')],
  hand=[(5, 5, 3), (4, 5, 3)], xc_auto=[(3, 16, 128, 32), (4, 16, 64, 16), (2, 5, 128, 32)], xc_update=[], xc_exact=False)


def ragged_regimes():
  """Channel counts that do not divide into the workgroups' groups (not a product shape: the product has 16 channels at 32
  and 64 samples; the kernel's `c1 = min(C, c0 + cper)` is what they exercise), for each mode, precision and geometry."""
  out = set()
  for H, h in ((128, 32), (64, 16)):
    for precision in (0, 1):
      for B, C in ((50, 16), (100, 7)):
        out |= xcorr_case_regimes(B, C, H, h, precision, force='0')
  assert all('ragged last channel group' in r for r in out)
  return out


def _show(regimes):
  return '\n'.join('  ' + ' '.join(str(v) for v in r) for r in sorted(regimes, key=str))


def test_the_gpu_suite_reaches_every_regime_of_the_update():
  need = D.product_regimes(32) | D.rollout_regimes(256) | ragged_regimes()
  # the mixed operand pairs of the backward under bf16 features and the rollout's one channel group are among them
  for H, h in ((128, 32), (64, 16)):
    assert ('xcorr toeplitz', 'd/dx', '%d/%d' % (H, h), 'bf16', 'channels/workgroup>1', 'even channel groups', 'one pass', 'f32 x bf16') in need
    assert ('xcorr toeplitz', 'd/dw', '%d/%d' % (H, h), 'bf16', 'channels/workgroup>1', 'even channel groups', 'one pass', 'bf16 x f32') in need
  for prec, pair in (('bf16', 'bf16 x bf16'), ('bf16x3', 'f32 x f32')):
    assert ('xcorr toeplitz', 'forward', '64/16', prec, 'channels/workgroup>1', 'even channel groups', 'one pass', pair) in need
    assert ('xcorr rows', prec, pair) in need
  missing = need - regimes_reached()
  assert not missing, 'dispatch regimes of the update that no GPU test reaches:\n' + _show(missing)
  # and by the tests of the single kernels alone: the whole net's test says that a gradient is off, theirs say which kernel's
  missing = need - regimes_reached(hand=[])
  assert not missing, 'dispatch regimes of the update that only the whole net\'s test reaches:\n' + _show(missing)


def test_the_product_reaches_what_the_small_batches_never_did():
  """The reason for the cases at the update's batch sizes, kept as a test: with batches of 1 - 6 only, these regimes of the
  product had no numeric test (and the check above names them)."""
  missing = D.product_regimes(32) - regimes_reached(**SMALL_BATCH_LISTS)
  print(_show(missing))
  for r in [('tconv', 9, 16, 2), ('tconv', 9, 16, 4), ('tconv', 1, 16, 2), ('tconv', 1, 16, 4),
            ('twrw', 9, 16, 1, 'tiles/group>1', 'no empty group'), ('twrw', 9, 16, 1, 'tiles/group>1', 'empty trailing groups'),
            ('twrw', 9, 16, 2, 'tiles/group>1', 'no empty group'),
            ('tact_bwd', 'pixb above minimum', 'contiguous', 'pool gradient'), ('tact_bwd', 'pixb above minimum', 'contiguous', 'no pool gradient'),
            ('tact_bwd', 'pixb above minimum', 'space-to-depth', 'no pool gradient')]:
    assert r in missing, r
  for mode in ('forward', 'd/dx', 'd/dw'):
    for geom in ('128/32', '64/16'):
      for prec in ('bf16', 'bf16x3'):
        r = ('xcorr toeplitz', mode, geom, prec, 'channels/workgroup>1', 'even channel groups',
             'two-pass sum' if mode == 'forward' else 'one pass', 'f32 x f32')
        # the one exception: test_xcorr_row_product_forward runs the forward at 200 samples on the Toeplitz kernel too
        assert (r in missing) != (r[1:4] == ('forward', '128/32', 'bf16x3')), r


def test_the_hand_worked_figures_of_the_update():
  """The arithmetic behind the regimes, at the product's shapes (a wrong restatement would move these)."""
  assert D.wrw_groups(9, 32, 128, 128, 16, 16)[0] == 512 and D.wrw_tiles(9, 32, 128, 128) == 2048           # 4 tiles per group
  assert D.wrw_groups(9, 32, 64, 64, 64, 32) == (256, 2) and D.wrw_tiles(9, 32, 64, 64) == 512             # 2 per group
  assert D.wrw_tiles(9, 32, 97, 97) == 1568 and D.wrw_groups(9, 32, 97, 97, 16, 16)[0] == 512              # per = 4: groups 392 .. 511 empty
  assert D.twrw_regime(9, 32, 97, 97, 1, 16)[-1] == 'empty trailing groups'
  assert D.tconv_cot(9, 64, 64, 64, 32) == 2 and D.tconv_cot(9, 32, 128, 128, 32) == 2                      # forward at 64^2, data gradient at 128^2
  assert D.tconv_cot(9, 32, 64, 64, 64) == 4                                                                 # data gradient of 64 -> 32 at 64^2
  assert D.tconv_cot(1, 64, 16, 16, 256) == 2 and D.tconv_cot(1, 32, 64, 64, 32) == 2                       # up2 forward, up0 data gradient
  assert D.tconv_cot(1, 64, 32, 32, 128) == 4 and D.tconv_cot(1, 64, 64, 64, 64) == 4                       # up1 / up0 forward
  assert D.act_pixb(32 * 128 * 128, 16) == 512 and D.act_pixb(32 * 97 * 97, 16) == 320 and D.act_pixb(6 * 128 * 128, 16) == 256
  assert D.channel_split(64, 16) == (4, 4) and D.channel_split(32, 16) == (2, 8) and D.channel_split(16, 16) == (1, 16)
  assert D.channel_split(200, 16) == (8, 2) and D.channel_split(50, 16) == (3, 6) and D.channel_split(100, 7) == (3, 3)
  assert D.channel_split(256, 16) == (16, 1) and D.channel_split(3, 1) == (1, 1) and D.channel_split(3, 16) == (1, 16)


def _every_case():
  """(taps, B, H, W, cin, cout) of every weight-gradient launch, (pixels, C) of every activation-gradient launch and (B, C) of
  every cross-correlation of the product and of the GPU tests' lists."""
  wrw, act, xc = set(), set(), set()
  for res_l, res_r in ((128, 32), (64, 16)):
    for l in D.net_layers(res_l, res_r):
      for B in (64, 32, 5, 3):
        wrw.add((l['taps'], B, l['r'], l['r'], l['cin'], l['cout']))
        act.add((B * l['r'] ** 2 * (4 if l['role'] == 'up' else 1), l['cout'] // 4 if l['role'] == 'up' else l['cout']))
  for cin, cout, B, H, W in TC.CONV3X3_CASES:
    wrw.add((9, B, H, W, cin, cout)); act.add((B * H * W, cout))
  for cin, cout, B, H, W in TC.CONVT_CASES:
    wrw.add((1, B, H, W, cin, 4 * cout)); act.add((4 * B * H * W, cout))
  for C, B, H, W, _ in TC.ACT_CASES:
    act.add((B * H * W, C))
  for B, C, H, h in TL.XCORR_AUTOGRAD_CASES + TL.XCORR_UPDATE_CASES + [(64, 16, 128, 32), (32, 16, 64, 16), (200, 16, 128, 32)] + \
      [(B, C, H, h) for H, h in TX.GEOMETRIES for B, C in TX.TOEPLITZ_BC + [(TX.LARGE_BATCH, 16)]]:
    xc.add((B, C, H, h))
  return sorted(wrw), sorted(act), sorted(xc)


def test_the_restatement_is_the_library_s_arithmetic():
  from stackrl_amd import build
  build.build()
  L = ctypes.CDLL(build.QLIB)       # host-side arithmetic only: no GPU call
  I32, I64 = ctypes.c_int32, ctypes.c_int64
  L.srl_twrw_scratch_floats.restype = I64
  L.srl_twrw_scratch_floats.argtypes = [I32] * 6
  L.srl_tact_bwd_blocks.restype = I32
  L.srl_tact_bwd_blocks.argtypes = [I64, I32]
  L.srl_tact_bwd_scratch_floats.restype = I64
  L.srl_tact_bwd_scratch_floats.argtypes = [I64, I32]
  L.srl_xcorr_mfma_scratch_bytes.restype = I64
  L.srl_xcorr_mfma_scratch_bytes.argtypes = [I32] * 6
  wrw, act, xc = _every_case()
  for taps, B, H, W, cin, cout in wrw:
    G, _ = D.wrw_groups(taps, B, H, W, cin, cout)
    assert L.srl_twrw_scratch_floats(B, H, W, cin, cout, taps) == G * taps * ((cin + 15) // 16 * 16) * cout, (taps, B, H, W, cin, cout)
  for npix, C in act:
    assert L.srl_tact_bwd_blocks(npix, C) == D.act_blocks(npix, C), (npix, C)
    assert L.srl_tact_bwd_scratch_floats(npix, C) == D.act_blocks(npix, C) * C, (npix, C)
  for B, C, H, h in xc:
    for mode in (0, 1, 2):
      for precision in (0, 1):
        assert L.srl_xcorr_mfma_scratch_bytes(mode, precision, B, C, H, h) == D.xcorr_scratch_bytes(mode, B, C, H, h), (mode, B, C, H, h)
