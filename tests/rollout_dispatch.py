"""The routing of the rollout (inference) forward, restated in plain Python (no GPU, no library call).

`qops.FastFeatures._unet` sends every layer of the two U-Nets to one of several kernels, and which one depends on the map
size, the dtype mode and the BATCH: the 16- / 32-output-channel layers go to csrc/conv_mfma.hip where the map is a multiple
of 16, the deep levels to the implicit GEMM of csrc/conv_gemm.hip where (cin, cout, W) is one of its instantiations and the
batch a multiple of the maps a workgroup takes, and whatever neither takes falls to a library convolution without bias plus
the fused passes of csrc/epilogue.hip.  Each function below names the PATH of one layer — a tuple of the kernel and the
quantities that pick its code path — so that a test can say which paths the product's rollout reaches
(`product_rollout_regimes`) and which ones a list of test cases reaches.  tests/test_rollout_dispatch.py holds the
restatement to the library's exports and the GPU suite's parameter lists to the product's paths;
tests/test_rollout_forward_gpu.py holds `forward_paths` to the calls a real forward makes."""

MODES = ('bf16', 'fp32-class', 'fp32 epilogues only')        # FastFeatures(): default; dtype=float32; dtype=float32, x3_conv=False
SHAPES = ((128, 32), (64, 16))                               # (res_left, res_right): Stack-v0, and resolution_factor=4


# ------------------------------------------------------------------------------------------------ csrc/conv_gemm.hip
def conv3x3_gemm_supported(cin, cout, W):
  if cout == 64:
    return (W in (32, 16) and cin in (32, 64, 128)) or (W == 8 and cin in (32, 64))
  if cout == 128:
    return W in (16, 8) and cin in (64, 128, 256)
  if cout == 256:
    return W in (8, 4) and cin in (128, 256)
  return False


def gemm_layers():
  """Every (cin, cout, W) the implicit GEMM is instantiated for."""
  return [(ci, co, w) for co in (64, 128, 256) for w in (32, 16, 8, 4) for ci in (32, 64, 128, 256) if conv3x3_gemm_supported(ci, co, w)]


def gemm_cfg(cout, W, x3=False):
  """`GemmCfg<COUT, W, X3>`: pixels per workgroup, whole maps per workgroup (NI), workgroups per map (PARTS), rows of a map
  per workgroup (RT), and SWZ (the swizzled 64-byte LDS pixel stride of the fp32-class 64-channel layers at 32^2)."""
  wm = cout // 64
  pxt = 128 * (4 // wm)
  ni = pxt // (W * W) if pxt >= W * W else 1
  return dict(PXT=pxt, NI=ni, PARTS=(W * W + pxt - 1) // pxt, RT=W if ni > 1 else pxt // W, SWZ=bool(x3 and cout == 64 and W == 32))


def conv3x3_gemm_batch_multiple(cout, W):
  return gemm_cfg(cout, W)['NI']


def conv3x3_gemm_wfrag_elems(cin, cout):
  return -1 if (cin % 32 or cout % 64) else (cin // 32) * 9 * (cout // 16) * 64 * 8


def gemm_workgroups(cout, W, B):
  c = gemm_cfg(cout, W)
  return B // c['NI'] if (c['NI'] > 1 or c['PXT'] == W * W) else B * c['PARTS']


def gemm_first_maps(cout, W, B):
  """`img0` of every workgroup of a launch."""
  c = gemm_cfg(cout, W)
  return sorted({(wg * c['NI']) if c['NI'] > 1 else wg // c['PARTS'] for wg in range(gemm_workgroups(cout, W, B))})


def gemm_regime(cin, cout, W, precision, B):
  """'multi-wg': some workgroup of the launch starts at a map other than the first (`img0 > 0`), so the kernel's map offset
  into the input, the output and — for NI > 1 — between the maps of one LDS tile are all in play."""
  assert conv3x3_gemm_supported(cin, cout, W) and B % conv3x3_gemm_batch_multiple(cout, W) == 0
  return ('conv_gemm', cin, cout, W, precision, 'multi-wg' if gemm_first_maps(cout, W, B)[-1] > 0 else 'one-wg')


def convt2x2_gemm_supported(cin, cout):
  return (cin, cout) in ((128, 64), (256, 128))


# ------------------------------------------------------------------------------------------------ csrc/conv_mfma.hip
def conv3x3_wfrag_elems(cin, cout):
  if cin not in (16, 32, 64) or cout not in (16, 32):
    return -1
  return (5 if cin == 16 else 9 * (cin // 32)) * (cout // 16) * 64 * 8


def convt2x2_wfrag_elems(cin, cout):
  if (cin, cout) not in ((32, 16), (64, 32), (128, 64), (256, 128)):
    return -1
  return (cin // 32) * (4 * cout // 16) * 64 * 8


# ------------------------------------------------------------------------------------------------ csrc/epilogue.hip
def epilogue_regime(kernel, dtype, form, npix, C, relu=True):
  """One launch of `k_bias_act` / `k_bias_act_pool` (a thread per 8 channels of a pixel — of a 2 x 2 block of pixels for the
  pool — in blocks of 256): the path tuple, and the launch's block structure."""
  n = (npix // 4 if kernel == 'bias_act_pool' else npix) * (C // 8)
  path = ('library+bias_act_pool', dtype) if kernel == 'bias_act_pool' else ('library+bias_act', dtype, form)
  return path, ('relu' if relu else 'no relu', 'one block' if n <= 256 else 'more blocks', 'partial last block' if n % 256 else 'full last block')


# ------------------------------------------------------------------------------------------------ qops.FastFeatures
def _unet_paths(res, cin0, depth, mode, B, filters=16):
  """`FastFeatures._unet` for one U-Net, layer by layer in call order."""
  bf16, x3 = mode == 'bf16', mode == 'fp32-class'
  hand = bf16 or x3
  dt = 'bf16' if bf16 else 'f32'
  prec = 'bf16' if bf16 else 'bf16x3'

  def mine(cin, cout, r):                 # `_mine`: csrc/conv_mfma.hip holds the layer and the map is whole 16 x 16 tiles
    return hand and cin in (16, 32, 64) and cout in (16, 32) and r % 16 == 0

  def gemm(cin, cout, r):                 # `_gemm`
    return hand and cout in (64, 128, 256) and cin % 32 == 0 and conv3x3_gemm_supported(cin, cout, r) and \
      B % conv3x3_gemm_batch_multiple(cout, r) == 0

  def conv(cin, cout, r, form='plain'):
    if mine(cin, cout, r):
      return [('conv_mfma', cin, cout, form, prec)]
    if gemm(cin, cout, r) and form != 'nchw':
      return [gemm_regime(cin, cout, r, prec, B)] + ([('pool2x2 slice', dt)] if form == 'slice+pool' else [])
    if form == 'slice+pool':
      return [('library+bias_act_pool', dt)]
    return [('library+bias_act', dt, 'nchw' if form == 'nchw' else 'in place')]

  out = []
  c, r = cin0, res
  for i in range(depth):
    f = filters * 2 ** i
    if i == 0 and x3 and f == 16 and r % 16 == 0:
      out.append(('thin+conv fused', c, 'uint8', 'slice+pool'))
    else:
      if i == 0 and hand:
        out.append(('thin', c, 'uint8', dt))
      else:
        out += conv(c, f, r)
      out += conv(f, f, r, 'slice+pool')
    c, r = f, r // 2
  fb = filters * 2 ** depth
  out += conv(c, fb, r) + conv(fb, fb, r)
  c = fb
  for i in range(depth - 1, -1, -1):
    f = filters * 2 ** i
    if hand and (c, f) in ((32, 16), (64, 32)) and r % 16 == 0:
      out.append(('convt_mfma', c, f, prec))
    elif hand and convt2x2_gemm_supported(c, f):
      out.append(('convt_gemm', c, f, prec))
    elif x3 and f % 4 == 0:
      out.append(('tconv 1x1 d2s', c, f))
    else:
      out.append(('library+bias_act', dt, 'slice'))
    r *= 2
    out += conv(2 * f, f, r) + conv(f, f, r, 'nchw' if i == 0 else 'plain')
    c = f
  return out


def pos_path(mode):
  return {'bf16': ('pos thin+project', 'bf16'), 'fp32-class': ('pos fused',), 'fp32 epilogues only': ('pos module',)}[mode]


def forward_paths(res_left, res_right, mode, B):
  """The path of every layer of `FastFeatures.__call__` (left U-Net, then the right one) and `.pos`, in call order, for B
  samples of `DeepQSiamFCN`'s default depths (4 and 2) and filters (16)."""
  assert mode in MODES
  return _unet_paths(res_left, 2, 4, mode, B) + _unet_paths(res_right, 1, 2, mode, B) + [pos_path(mode)]


def batch_class(B):
  """The largest batch multiple of a gemm layer (8, 4, 2, 1) that divides B: all of the batch that the routing looks at."""
  return max(m for m in (8, 4, 2, 1) if B % m == 0)


def forward_regime(res_left, res_right, mode, B):
  """One whole forward: which layers the gemm takes is a function of the shape, the mode and `batch_class(B)`."""
  return ('forward', '{}/{}'.format(res_left, res_right), mode, 'batch multiple of {}'.format(batch_class(B)))


def has_library_call(paths):
  return any(p[0].startswith('library') or p[0] == 'pos module' for p in paths)


def policy_chunks(B, chunk):
  """The batches `FusedPolicy(chunk=chunk)` hands the forward for one call over B samples."""
  return [min(B, s + chunk) - s for s in range(0, B, chunk)]


# ------------------------------------------------------------------------------------------------ the product
# bench.py `dqn_shape` / BASELINE.json configs[2..4]: the envs of a rank, held as `groups = 2` handles (`dqn_leg`), each
# evaluated by one `FusedPolicy(chunk=2048)` call
PRODUCT_RANKS = {(128, 32): (4096, 2048), (64, 16): (2048,)}      # configs[2] and configs[3]; configs[4]
PRODUCT_GROUPS, PRODUCT_CHUNK = 2, 2048
RAGGED_BATCH = 7                                                  # B % 8 != 0 and odd: the batch a user's n_parallel can give


def product_batches(shape):
  out = set()
  for envs in PRODUCT_RANKS[shape]:
    out |= set(policy_chunks(envs // PRODUCT_GROUPS, PRODUCT_CHUNK))
  return sorted(out) + [RAGGED_BATCH]


def product_rollout_regimes():
  """The union of layer paths, and the whole-forward routings, of the benchmark's rollout calls: both shapes, bf16 and
  fp32-class, the per-call batches of the configs, and one ragged batch per shape (every gemm layer with a batch multiple
  above 1 falls to the library)."""
  out = set()
  for shape in SHAPES:
    for mode in ('bf16', 'fp32-class'):
      for B in product_batches(shape):
        out |= set(forward_paths(shape[0], shape[1], mode, B))
        out.add(forward_regime(shape[0], shape[1], mode, B))
  return out


def forward_check(what, shape, mode):
  return (what, '{}/{}'.format(*shape), mode)


def product_forward_checks():
  """What the suite asks of the whole forward besides its comparison with float64, per shape and mode of the product: that a
  sample's result does not depend on its position in the batch, and that `FusedPolicy`'s chunking does not change its actions."""
  return {forward_check(what, shape, mode) for what in ('position independence', 'policy chunks') for shape in SHAPES
          for mode in ('bf16', 'fp32-class')}
