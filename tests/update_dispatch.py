"""The host-side choices of the update's kernels, restated in plain Python (no GPU, no library call).

The host code of csrc/train_conv.hip and csrc/xcorr_mfma.hip picks template instantiations and loop structures from the
BATCH SIZE: how many output-channel tiles a `k_tconv` workgroup takes (`launch_conv`), how many pixel tiles a `k_twrw` group
reduces and whether trailing groups are left without one (`wrw_groups`), how many pixels a `k_tact_bwd` block takes
(`bias_grad_pixb`), how many channels a `k_xcorr_mfma` workgroup loops over (`channel_split`).  Each function below names the
REGIME of one launch — the tuple of those choices — so that a test can say which regimes the product's update reaches
(`product_regimes`) and which ones a list of test cases reaches.  tests/test_update_dispatch.py holds the restatement to the
library wherever the library exports the quantity, and the GPU suite's parameter lists to the product's regimes."""


# ------------------------------------------------------------------------------------------------ csrc/train_conv.hip
def conv_tw(taps, H, W):
  """Tile width of the pixel tiles: 16 (one sample, 16 x 16 pixels; the 1 x 1 kernel's 256 consecutive pixels), or 8 (four
  samples of 8 x 8) for maps of at most 8 x 8."""
  return 16 if (taps == 1 or W > 8 or H > 8) else 8


def wrw_tiles(taps, B, H, W):
  if taps == 1:
    return (B * H * W + 255) // 256
  if W > 8 or H > 8:
    return B * ((H + 15) // 16) * ((W + 15) // 16)
  return ((B + 3) // 4) * ((H + 7) // 8) * ((W + 7) // 8)


def wrw_groups(taps, B, H, W, cin, cout):
  tiles = wrw_tiles(taps, B, H, W)
  cot = 4 if cout % 64 == 0 else 2 if cout % 32 == 0 else 1
  blocks = ((cin + 15) // 16) * (cout // (cot * 16))
  return int(min(max(1024 // blocks, 1), tiles, 512)), cot


def tconv_cot(taps, B, H, W, cout):
  """`launch_conv`: 64 output channels per workgroup when that still gives 512 workgroups, else 32, else 16.  The library
  does not export this choice; profiles/update_batch_tests_kernel_names.txt, the kernel-name summary of a traced run of the
  update-path GPU tests, lists k_tconv with COT 1, 2 and 4 for both tap counts."""
  tiles = wrw_tiles(taps, B, H, W)          # the same pixel tiling as the weight gradient's
  if cout % 64 == 0 and tiles * (cout // 64) >= 512:
    return 4
  if cout % 32 == 0 and tiles * (cout // 32) >= 512:
    return 2
  return 1


def tconv_regime(taps, B, H, W, cout):
  return ('tconv', taps, conv_tw(taps, H, W), tconv_cot(taps, B, H, W, cout))


def twrw_regime(taps, B, H, W, cin, cout):
  G, cot = wrw_groups(taps, B, H, W, cin, cout)
  tiles = wrw_tiles(taps, B, H, W)
  per = (tiles + G - 1) // G
  return ('twrw', taps, conv_tw(taps, H, W), cot, 'tiles/group>1' if per > 1 else 'tiles/group=1',
          'empty trailing groups' if (G - 1) * per >= tiles else 'no empty group')


def act_pixb(npix, C):
  ppi = 256 // (C // 4)
  pixb = max((npix + 1023) // 1024, 4 * ppi)
  return (pixb + ppi - 1) // ppi * ppi


def act_blocks(npix, C):
  pixb = act_pixb(npix, C)
  return (npix + pixb - 1) // pixb


def tact_regime(B, H, W, C, s2d=False, pool=False):
  """(H, W) is the map the gradient arrives on (for the space-to-depth form: the transposed convolution's OUTPUT map)."""
  return ('tact_bwd', 'pixb above minimum' if act_pixb(B * H * W, C) > 4 * (256 // (C // 4)) else 'pixb minimum',
          'space-to-depth' if s2d else 'contiguous', 'pool gradient' if pool else 'no pool gradient')


# ------------------------------------------------------------------------------------------------ csrc/xcorr_mfma.hip
def channel_split(B, C):
  want = max(1, min(C, (256 + B - 1) // B))
  cper = (C + want - 1) // want
  return cper, (C + cper - 1) // cper


def xcorr_scratch_bytes(mode, B, C, H, kh):
  _, csplit = channel_split(B, C)
  O = H - kh + 1
  return B * csplit * O * O * 4 if (mode == 0 and csplit > 1) else 0


F32, BF16 = 'f32', 'bf16'                # operand dtypes: a launch's pair is (map, kernel)


def xcorr_rows_chosen(mode, precision, B, C, H, kh, pair=(F32, F32), force=None):
  """`use_rows`: the row-product forward (float32 or bf16 operands of one kind) for 128 / 32 at 192 samples and more; `force`
  is the SRL_XCORR_ROWS setting of the call ('0', '1' or None).  The forward entry points of qops.py pass no mixed pair;
  `_XCorrMFMA.backward` does, under bf16 features (`backward_pairs`), and a mixed pair never takes this kernel."""
  if mode != 0 or H != 128 or kh != 32 or C < 1 or C > 16 or pair[0] != pair[1] or (precision == 1 and pair[0] != F32):
    return False
  if force in ('0', '1'):
    return force == '1'
  return B >= 192


def xcorr_regime(mode, precision, B, C, H, kh, pair=(F32, F32), force=None):
  """`launch` instantiates the Toeplitz kernel per operand pair (precision 1 takes float32 operands only), so the pair is
  part of the regime."""
  assert precision == 0 or pair == (F32, F32)
  if xcorr_rows_chosen(mode, precision, B, C, H, kh, pair, force):
    return ('xcorr rows', 'bf16x3' if precision else 'bf16', '{} x {}'.format(*pair))
  cper, csplit = channel_split(B, C)
  return ('xcorr toeplitz', ('forward', 'd/dx', 'd/dw')[mode], '{}/{}'.format(H, kh), 'bf16x3' if precision else 'bf16',
          'channels/workgroup>1' if cper > 1 else 'channels/workgroup=1',
          'ragged last channel group' if C % cper else 'even channel groups',
          'two-pass sum' if (mode == 0 and csplit > 1) else 'one pass', '{} x {}'.format(*pair))


def backward_pairs(features):
  """The (map, kernel) pair of each mode as `_XCorrMFMA` launches it at precision 0 with features of one dtype: the output
  gradient is float32 whatever the features are, so under bf16 features d/dx takes a float32 padded gradient with bf16
  flipped kernels and d/dw bf16 maps with a float32 gradient."""
  return {0: (features, features), 1: (F32, features), 2: (features, F32)}


# ------------------------------------------------------------------------------------------------ the network
def net_layers(res_left=128, res_right=32):
  """Every convolution `HandNet` runs (qtrain.py; nets.py / layers.py:135-259), as dicts: taps, the INPUT map side r, cin,
  cout (4 f for the transposed layers' 1 x 1 form), the role in the U-Net, and whether the backward takes the data gradient
  (`need_dx`: not for a U-Net's first layer)."""
  out = []
  for res, cin0, depth in ((res_left, 2, 4), (res_right, 1, 2)):
    c, r = cin0, res
    for i in range(depth):
      f = 16 * 2 ** i
      out += [dict(taps=9, r=r, cin=c, cout=f, role='down0', need_dx=i > 0), dict(taps=9, r=r, cin=f, cout=f, role='down1', need_dx=True)]
      c, r = f, r // 2
    fb = 16 * 2 ** depth
    out += [dict(taps=9, r=r, cin=c, cout=fb, role='bottom', need_dx=True), dict(taps=9, r=r, cin=fb, cout=fb, role='bottom', need_dx=True)]
    c = fb
    for i in range(depth - 1, -1, -1):
      f = 16 * 2 ** i
      out.append(dict(taps=1, r=r, cin=c, cout=4 * f, role='up', need_dx=True))     # up{i}: 1 x 1 to 4 f channels (depth-to-space)
      r *= 2
      out += [dict(taps=9, r=r, cin=2 * f, cout=f, role='dec', need_dx=True), dict(taps=9, r=r, cin=f, cout=f, role='dec', need_dx=True)]
      c = f
  o = res_left - res_right + 1
  out += [dict(taps=9, r=o, cin=1, cout=16, role='pos', need_dx=True), dict(taps=9, r=o, cin=16, cout=16, role='pos', need_dx=True)]   # pos_layers
  return out


def net_shapes():
  """(taps, H, cin, cout) of every convolution `HandNet` differentiates at 128 / 32 inputs."""
  return [(l['taps'], l['r'], l['cin'], l['cout']) for l in net_layers()]


def layer_regimes(l, B, n):
  """The regimes of one layer in an update: forward at B samples, the three backward passes at n."""
  taps, r, cin, cout = l['taps'], l['r'], l['cin'], l['cout']
  out = {tconv_regime(taps, B, r, r, cout), twrw_regime(taps, n, r, r, cin, cout)}
  if l['role'] == 'up':
    out.add(tact_regime(n, 2 * r, 2 * r, cout // 4, s2d=True))
    if l['need_dx']:
      out.add(tconv_regime(1, n, r, r, cin))
  else:
    out.add(tact_regime(n, r, r, cout, pool=l['role'] == 'down1'))
    if l['need_dx']:
      out.add(tconv_regime(9, n, r, r, (cin + 15) // 16 * 16))
  return out


def product_regimes(minibatch=32):
  """What one Double-DQN update of `minibatch` transitions launches: the online net forward on 2 x minibatch samples
  (states and next states in one pass), the target net on minibatch, the backward on the first minibatch; for the Stack-v0
  shapes (128 / 32) and the 64 x 64 configuration (64 / 16); the cross-correlation in both precisions — at precision 0 with
  float32 features and with bf16 features, whose backward launches the mixed operand pairs."""
  out = set()
  for res_l, res_r in ((128, 32), (64, 16)):
    for l in net_layers(res_l, res_r):
      out |= layer_regimes(l, 2 * minibatch, minibatch)
      out.add(tconv_regime(l['taps'], minibatch, l['r'], l['r'], l['cout']))          # the target net
    for precision, features in ((0, F32), (1, F32), (0, BF16)):
      pairs = backward_pairs(features)
      out.add(xcorr_regime(0, precision, 2 * minibatch, 16, res_l, res_r, pairs[0]))
      for mode in (0, 1, 2):
        out.add(xcorr_regime(mode, precision, minibatch, 16, res_l, res_r, pairs[mode]))
  return out


def rollout_regimes(chunk=256):
  """The cross-correlation forward of the rollout at a policy chunk of `chunk` samples (256 and more), bf16 features under
  autocast or float32 features with the split.  128 / 32 takes the row-product kernel; 64 / 16 has none and runs the Toeplitz
  forward with ONE CHANNEL GROUP: a workgroup loops over all 16 channels and writes the output itself, in one pass."""
  out = set()
  for res_l, res_r in ((128, 32), (64, 16)):
    out |= {xcorr_regime(0, 0, chunk, 16, res_l, res_r, (BF16, BF16)), xcorr_regime(0, 1, chunk, 16, res_l, res_r)}
  assert channel_split(chunk, 16) == (16, 1)
  return out
