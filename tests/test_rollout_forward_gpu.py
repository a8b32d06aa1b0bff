"""GPU tests of the rollout (inference) forward at every layer path the product's shapes reach: each instantiation of the
implicit-GEMM convolution past its first workgroup, the passes of csrc/epilogue.hip bit for bit, and `qops.FastFeatures` /
`FusedPolicy` at 128 / 32 and 64 / 16 against the same module in float64 with the routing asserted call by call
(tests/rollout_dispatch.py restates the routing; tests/test_rollout_dispatch.py holds the lists below to the product)."""
import copy
import functools

import pytest

import rollout_dispatch as D

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

_CL = torch.channels_last


# ------------------------------------------------------------------------------------------------ C1: csrc/conv_gemm.hip
# (cin, cout, W, B): every instantiation at twice its batch multiple — two workgroups per row block, the second at `img0 = B / 2`
GEMM_TWO_GROUP_CASES = [(32, 64, 32, 2), (64, 64, 32, 2), (128, 64, 32, 2), (64, 128, 16, 2), (128, 128, 16, 2), (256, 128, 16, 2),
                        (32, 64, 16, 4), (64, 64, 16, 4), (128, 64, 16, 4), (128, 256, 8, 4), (256, 256, 8, 4),
                        (64, 128, 8, 8), (128, 128, 8, 8), (256, 128, 8, 8),
                        (32, 64, 8, 16), (64, 64, 8, 16), (128, 256, 4, 16), (256, 256, 4, 16)]
# (cin, cout, B, H, W): 210 and 162 pixels (two pixel tiles of 128, the last one partial, the second half starting inside a
# tile), and 512 (whole tiles)
CONVT_GEMM_POSITION_CASES = [(128, 64, 6, 5, 7), (256, 128, 2, 9, 9), (256, 128, 8, 8, 8)]


@pytest.mark.parametrize('cin,cout,W,B', GEMM_TWO_GROUP_CASES)
@pytest.mark.parametrize('f32', [False, True])
def test_conv3x3_gemm_past_the_first_workgroup(cin, cout, W, B, f32):
  """`k_conv3x3_gemm` at twice the layer's batch multiple, so that a workgroup starts at a map other than the first: against
  float64 torch on the same operands with the reference and tolerances of test_conv3x3_gemm_matches_torch_fp64 (2^-8
  relative above a floor of 1e-2 of the scale for bf16, 3e-5 of the scale for the fp32-class form), and position
  independence bit for bit — each half of the batch run alone gives that half of the whole call's output (fixed-order sums)."""
  from stackrl_amd import qops
  g = torch.Generator(device='cuda').manual_seed(cin + cout + W)
  dt = torch.float32 if f32 else torch.bfloat16
  x = torch.randn(B, cin, W, W, generator=g, device='cuda').to(dt).contiguous(memory_format=_CL)
  w = torch.randn(cout, cin, 3, 3, generator=g, device='cuda') / (3 * cin ** 0.5)
  b = torch.randn(cout, generator=g, device='cuda') * 0.1
  wr = w if f32 else w.to(torch.bfloat16).float()
  ref = torch.relu(torch.nn.functional.conv2d(x.double(), wr.double(), b.double(), padding=1))
  m = B // 2
  assert qops.conv3x3_gemm_supported(cin, cout, W, B) and qops.conv3x3_gemm_supported(cin, cout, W, m)
  assert not qops.conv3x3_gemm_supported(cin, cout, W, m + 1) or m == 1
  wf = qops.pack_conv3x3_gemm_weights(w, x3=f32)
  y = qops.conv3x3_gemm_bias_relu(x, wf, b, cout)
  scale = float(ref.abs().max())
  err = (y.double() - ref).abs()
  print('max error / scale', float(err.max()) / scale)
  if f32:
    assert y.dtype == torch.float32 and float(err.max()) <= 3e-5 * scale
  else:
    assert y.dtype == torch.bfloat16 and bool((err <= 2.0 ** -8 * ref.abs().clamp(min=1e-2 * scale)).all())
  for s in (slice(0, m), slice(m, B)):
    assert torch.equal(qops.conv3x3_gemm_bias_relu(x[s], wf, b, cout), y[s])
  cat = torch.full((B, 2 * cout, W, W), 3.0, device='cuda', dtype=dt).contiguous(memory_format=_CL)
  qops.conv3x3_gemm_bias_relu(x, wf, b, cout, out=cat, out_offset=cout)
  assert torch.equal(cat[:, cout:], y) and bool((cat[:, :cout] == 3.0).all())


@pytest.mark.parametrize('cin,cout,B,H,W', CONVT_GEMM_POSITION_CASES)
@pytest.mark.parametrize('f32', [False, True])
def test_convt2x2_gemm_is_position_independent(cin, cout, B, H, W, f32):
  """`k_convt2x2_gemm` over more than one pixel tile: float64 torch with the tolerances of
  test_convt2x2_gemm_matches_torch_fp64, and each half of the batch run alone equal bit for bit to that half of the whole
  call (the second half starts inside a pixel tile where B H W / 2 is no multiple of 128)."""
  from stackrl_amd import qops
  F = torch.nn.functional
  g = torch.Generator(device='cuda').manual_seed(cin + H)
  dt = torch.float32 if f32 else torch.bfloat16
  x = torch.randn((B, cin, H, W), generator=g, device='cuda').to(dt).contiguous(memory_format=_CL)
  w = torch.randn((cin, cout, 2, 2), generator=g, device='cuda') / cin ** 0.5
  b = torch.randn(cout, generator=g, device='cuda') * 0.1
  wr = w if f32 else w.to(torch.bfloat16).float()
  ref = F.relu(F.conv_transpose2d(x.double(), wr.double(), b.double(), stride=2))
  wf = qops.pack_convt2x2_weights(w, x3=f32)

  def run(xs):
    cat = torch.full((xs.shape[0], 2 * cout, 2 * H, 2 * W), 3.0, device='cuda', dtype=dt).contiguous(memory_format=_CL)
    return qops.convt2x2_gemm_bias_relu(xs, wf, b, cout, cat, 0)
  cat = run(x)
  assert B * H * W > 128
  err = (cat[:, :cout].double() - ref).abs()
  if f32:
    assert float(err.max()) <= 3e-5 * float(ref.abs().max())
  else:
    assert bool((err <= 2.0 ** -8 * ref.abs().clamp(min=1e-2 * float(ref.abs().max()))).all())
  assert bool((cat[:, cout:] == 3.0).all())
  m = B // 2
  for s in (slice(0, m), slice(m, B)):
    assert torch.equal(run(x[s]), cat[s])


# ------------------------------------------------------------------------------------------------ C2: csrc/epilogue.hip
EPILOGUE_DTYPES = ('bf16', 'f32')
BIAS_ACT_FORMS = ('in place', 'slice', 'nchw')
EPILOGUE_CHANNELS = (8, 32, 64)
POOL_MAPS = ((8, 8), (4, 6))
BIAS_ACT_MAPS = POOL_MAPS + ((5, 7),)
EPILOGUE_BATCH = 3
_TIE_BIAS = 2.0 ** -8
# bf16 bit patterns of 1, 1 + 2^-7, -(1 + 2^-7), -1: with the bias 2^-8 the float32 sums of the first three lie half-way between
# two bf16 values (round to even: 0x3f80, 0x3f82, 0xbf80), the last gives -(1 - 2^-8), which bf16 holds
_TIE_BITS = (0x3f80, 0x3f81, 0xbf81, 0xbf80)


def _epilogue_operands(C, H, W, dt):
  """Convolution output [3, C, H, W] channels-last and a float32 bias: normal values of both signs, and in channel 1 of the
  first sample the hand-built values whose sum with the bias is a rounding tie in bf16."""
  g = torch.Generator(device='cuda').manual_seed(C + 10 * H + W)
  y = torch.randn((EPILOGUE_BATCH, C, H, W), generator=g, device='cuda').to(dt).contiguous(memory_format=_CL)
  b = torch.randn(C, generator=g, device='cuda') * 0.5
  b[1] = _TIE_BIAS
  ties = torch.tensor([v - 65536 if v >= 32768 else v for v in _TIE_BITS], dtype=torch.int16, device='cuda').view(torch.bfloat16)
  y[0, 1, 0, :4] = ties.to(dt)
  s = (y[0, 1, 0, :3].float() + _TIE_BIAS).view(torch.int32) & 0xffff
  assert bool((s == 0x8000).all())              # half a bf16 unit in the last place, exactly
  assert bool(((y.float() + b.view(1, C, 1, 1)) < 0).any())
  return y, b


def _epilogue_reference(y, b, relu, dt):
  r = y.float() + b.view(1, -1, 1, 1)
  return (r.relu() if relu else r).to(dt)


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('H,W', BIAS_ACT_MAPS)
@pytest.mark.parametrize('C', EPILOGUE_CHANNELS)
@pytest.mark.parametrize('form', BIAS_ACT_FORMS)
@pytest.mark.parametrize('dtype', EPILOGUE_DTYPES)
def test_bias_act_is_exact(dtype, form, C, H, W, relu):
  """`k_bias_act` is one float32 add, a max and one round-to-nearest-even: equal bit for bit to torch's
  `(x.float() + b).relu().to(dtype)` in each output form (in place; a channel slice of a wider buffer with the rest untouched;
  NCHW), with and without the ReLU, on one block and on several."""
  from stackrl_amd import qops
  dt = torch.bfloat16 if dtype == 'bf16' else torch.float32
  y, b = _epilogue_operands(C, H, W, dt)
  ref = _epilogue_reference(y, b, relu, dt)
  if dtype == 'bf16':
    want = torch.tensor([0x3f80, 0x3f82, 0xbf80 - 65536], dtype=torch.int16, device='cuda').view(torch.bfloat16).float()
    assert torch.equal(ref[0, 1, 0, :3].float(), want.relu() if relu else want)        # the reference itself rounds ties to even
  if form == 'in place':
    src = y.clone(memory_format=torch.preserve_format)
    got = qops.bias_act(src, b, relu=relu)
    assert got is src and torch.equal(got, ref)
  elif form == 'slice':
    buf = torch.full((EPILOGUE_BATCH, C + 16, H, W), 3.0, device='cuda', dtype=dt).contiguous(memory_format=_CL)
    src = y.clone(memory_format=torch.preserve_format)
    qops.bias_act(src, b, out=buf, out_offset=8, relu=relu)
    assert torch.equal(buf[:, 8:8 + C], ref) and bool((buf[:, :8] == 3.0).all()) and bool((buf[:, 8 + C:] == 3.0).all())
    assert torch.equal(src, y)
  else:
    got = qops.bias_act(y, b, relu=relu, nchw=True)
    assert got.is_contiguous() and got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize('H,W', POOL_MAPS)
@pytest.mark.parametrize('C', EPILOGUE_CHANNELS)
@pytest.mark.parametrize('dtype', EPILOGUE_DTYPES)
def test_bias_act_pool_is_exact(dtype, C, H, W):
  """`k_bias_act_pool`: the skip slice equal bit for bit to `(x.float() + b).relu().to(dtype)`, the other half of the buffer
  untouched, and the pooled tensor equal to the 2 x 2 max-pool of the STORED skip tensor."""
  from stackrl_amd import qops
  dt = torch.bfloat16 if dtype == 'bf16' else torch.float32
  y, b = _epilogue_operands(C, H, W, dt)
  ref = _epilogue_reference(y, b, True, dt)
  skip = torch.full((EPILOGUE_BATCH, 2 * C, H, W), 3.0, device='cuda', dtype=dt).contiguous(memory_format=_CL)
  pooled = qops.bias_act_pool(y, b, skip, C)
  assert torch.equal(skip[:, C:], ref) and bool((skip[:, :C] == 3.0).all())
  assert pooled.shape == (EPILOGUE_BATCH, C, H // 2, W // 2) and pooled.is_contiguous(memory_format=_CL)
  assert torch.equal(pooled, torch.nn.functional.max_pool2d(ref.float(), 2).to(dt))


def test_epilogue_argument_checks():
  """Offsets or strides that are no multiples of 8, an odd map for the pool, and pool + NCHW of the convolution kernel return
  the error code and set the message; the output buffers stay as they were."""
  from stackrl_amd import qops
  L = qops.load()
  y = torch.zeros((2, 16, 5, 6), device='cuda', dtype=torch.bfloat16).contiguous(memory_format=_CL)
  yf = y.float().contiguous(memory_format=_CL)
  b = torch.ones(16, device='cuda')
  out = torch.full((2, 40, 6, 6), 3.0, device='cuda', dtype=torch.float32).contiguous(memory_format=_CL)   # room for either dtype
  st = qops._stream(y)
  for fn, src, name in ((L.srl_bias_act, y, b'srl_bias_act:'), (L.srl_bias_act_f32, yf, b'srl_bias_act_f32:')):
    for stride, off, C, hw in ((40, 4, 16, 0), (36, 8, 16, 0), (40, 8, 12, 0), (16, 0, 16, 7)):
      assert fn(src.data_ptr(), out.data_ptr(), b.data_ptr(), 60, C, stride, off, hw, 1, st) == 1
      assert L.srl_epilogue_last_error().startswith(name)
  pooled = torch.full((2, 16, 3, 3), 3.0, device='cuda', dtype=torch.float32).contiguous(memory_format=_CL)
  for fn, src, name in ((L.srl_bias_act_pool, y, b'srl_bias_act_pool:'), (L.srl_bias_act_pool_f32, yf, b'srl_bias_act_pool_f32:')):
    for H, W, stride, off in ((5, 6, 40, 8), (6, 5, 40, 8), (6, 4, 36, 8), (6, 4, 40, 4)):
      assert fn(src.data_ptr(), out.data_ptr(), pooled.data_ptr(), b.data_ptr(), 2, H, W, 16, stride, off, st) == 1
      assert L.srl_epilogue_last_error().startswith(name)
  with pytest.raises(RuntimeError, match='srl_bias_act'):
    qops.bias_act(y, b, out=out.to(torch.bfloat16).contiguous(memory_format=_CL), out_offset=4)
  x = torch.zeros((1, 16, 16, 16), device='cuda', dtype=torch.bfloat16).contiguous(memory_format=_CL)
  w = qops.pack_conv3x3_weights(torch.zeros(16, 16, 3, 3, device='cuda'))
  with pytest.raises(RuntimeError, match='srl_conv3x3_bias_relu'):
    qops.conv3x3_bias_relu(x, w, b, 16, pool=True, nchw=True)
  torch.cuda.synchronize()
  assert bool((out == 3.0).all()) and bool((pooled == 3.0).all())


# ------------------------------------------------------------------------------------------------ C3: the forward
_BF16, _X3 = 'bf16', 'fp32-class'
FORWARD_CASES = [(shape, mode, B) for shape in D.SHAPES for mode in (_BF16, _X3) for B in (8, D.RAGGED_BATCH)]
INDEPENDENCE_CASES = [(shape, mode) for shape in D.SHAPES for mode in (_BF16, _X3)]
INDEPENDENCE_BATCH = 16
POLICY_CASES = INDEPENDENCE_CASES
POLICY_BATCH, POLICY_CHUNKS = 20, (8, 32)
_SAMPLES = 20


def _case_id(case):
  return '-'.join('{}/{}'.format(*v) if isinstance(v, tuple) else str(v).replace(' ', '_') for v in case)


class _Trace(object):
  """Recording wrappers round the entry points `FastFeatures` can send a layer to; while `on`, every call is noted as the path
  tuple tests/rollout_dispatch.py gives that layer (a library convolution is noted together with the epilogue pass behind it)."""

  def __init__(self, monkeypatch):
    from stackrl_amd import qops, qtrain
    self.paths, self.on, self._lib = [], False, None
    F = torch.nn.functional
    for mod, name in [(qops, n) for n in ('conv3x3_bias_relu', 'thin_conv3x3_bias_relu', 'conv3x3_thin', 'conv3x3_gemm_bias_relu', 'bias_act',
                                         'bias_act_pool', 'pool2x2', 'convt2x2_bias_relu', 'convt2x2_gemm_bias_relu',
                                         'conv3x3_relu_project', 'thin_conv3x3_relu_project')] + \
                     [(qtrain, 'tconv'), (F, 'conv2d'), (F, 'conv_transpose2d')]:
      monkeypatch.setattr(mod, name, self._wrap(name, getattr(mod, name)))

  def _wrap(self, name, fn):
    @functools.wraps(fn)
    def wrapper(*a, **kw):
      if self.on:
        getattr(self, '_' + name)(*a, **kw)
      return fn(*a, **kw)
    return wrapper

  def record(self):
    trace = self

    class _On(object):
      def __enter__(self):
        trace.paths, trace.on, trace._lib = [], True, None

      def __exit__(self, *exc):
        trace.on = False
        assert trace._lib is None
    return _On()

  @staticmethod
  def _dt(t):
    return {torch.bfloat16: 'bf16', torch.float32: 'f32'}[t.dtype]

  @staticmethod
  def _prec(t):
    return {torch.bfloat16: 'bf16', torch.float32: 'bf16x3'}[t.dtype]

  def _note(self, path):
    assert self._lib is None, 'a library convolution without an epilogue pass behind it'
    self.paths.append(path)

  def _conv3x3_bias_relu(self, x, wfrag, bias, cout, out=None, out_offset=0, pool=False, nchw=False):
    assert not pool or (out is not None and out_offset == cout)
    self._note(('conv_mfma', x.shape[1], cout, 'nchw' if nchw else 'slice+pool' if pool else 'plain', self._prec(x)))

  def _thin_conv3x3_bias_relu(self, x, w1, b1, wfrag, bias, out=None, out_offset=0, pool=False, nchw=False):
    assert pool and out is not None and out_offset == 16 and not nchw
    self._note(('thin+conv fused', x.shape[3], {torch.uint8: 'uint8'}[x.dtype], 'slice+pool'))

  def _conv3x3_thin(self, x, w, bias, out=None, dtype=torch.bfloat16):
    if out is None:
      self._note(('thin', x.shape[3], {torch.uint8: 'uint8'}[x.dtype], {torch.bfloat16: 'bf16', torch.float32: 'f32'}[dtype]))
    else:                              # the position head's first layer, into the zero-margined map
      self._note(('pos thin', self._dt(out)))

  def _conv3x3_relu_project(self, x, *a, **kw):
    assert self.paths.pop() == ('pos thin', self._dt(x))
    self._note(('pos thin+project', self._dt(x)))

  def _thin_conv3x3_relu_project(self, *a, **kw):
    self._note(('pos fused',))

  def _conv3x3_gemm_bias_relu(self, x, wfrag, bias, cout, out=None, out_offset=0):
    self._note(D.gemm_regime(x.shape[1], cout, x.shape[3], self._prec(x), x.shape[0]))

  def _pool2x2(self, buf, C, offset=0):
    self._note(('pool2x2 slice', self._dt(buf)))

  def _convt2x2_bias_relu(self, x, wfrag, bias, cout, out, out_offset=0):
    self._note(('convt_mfma', x.shape[1], cout, self._prec(x)))

  def _convt2x2_gemm_bias_relu(self, x, wfrag, bias, cout, out, out_offset=0):
    self._note(('convt_gemm', x.shape[1], cout, self._prec(x)))

  def _tconv(self, x, wp, bias, cout, taps=9, relu=True, out=None, d2s=0):
    assert taps == 1 and relu and d2s and cout == 4 * d2s
    self._note(('tconv 1x1 d2s', x.C, d2s))

  def _conv2d(self, *a, **kw):
    assert self._lib is None
    self._lib = 'conv'

  def _conv_transpose2d(self, *a, **kw):
    assert self._lib is None
    self._lib = 'transposed'

  def _bias_act(self, y, bias, out=None, out_offset=0, relu=True, nchw=False):
    form = 'nchw' if nchw else 'in place' if out is None else 'slice'
    assert relu and self._lib == ('transposed' if form == 'slice' else 'conv'), (form, self._lib)
    self._lib = None
    self._note(('library+bias_act', self._dt(y), form))

  def _bias_act_pool(self, y, bias, skip, skip_offset):
    assert self._lib == 'conv'
    self._lib = None
    self._note(('library+bias_act_pool', self._dt(y)))


@functools.lru_cache(maxsize=None)
def _net(shape):
  """`DeepQSiamFCN` for the shape, with biases that are not zero (the initialiser's are: a wrong bias add would be invisible)."""
  from stackrl_amd import nets
  net = nets.DeepQSiamFCN(input_spec=((shape[0], shape[0], 2), (shape[1], shape[1], 1)), seed=5).cuda().eval()
  g = torch.Generator().manual_seed(6)
  with torch.no_grad():
    for m in net.modules():
      if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
        m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
  return net


@functools.lru_cache(maxsize=None)
def _observations(shape):
  g = torch.Generator().manual_seed(4)
  xm = torch.randint(0, 256, (_SAMPLES, shape[0], shape[0], 2), generator=g, dtype=torch.uint8)
  xo = torch.randint(0, 256, (_SAMPLES, shape[1], shape[1], 1), generator=g, dtype=torch.uint8)
  return xm, xo


def _xcorr64(x, w):
  """`layers.correlation` in float64 by the correlation theorem: x [B,C,H,H], w [B,C,h,h] -> [B,1,H-h+1,H-h+1] (the circular
  correlation of the zero-padded kernel has no wrapped term at shifts up to H - h)."""
  H, h = x.shape[-1], w.shape[-1]
  c = torch.fft.irfft2(torch.fft.rfft2(x) * torch.fft.rfft2(w, s=(H, H)).conj(), s=(H, H)).sum(1, keepdim=True)
  return c[..., :H - h + 1, :H - h + 1]


@functools.lru_cache(maxsize=None)
def _reference(shape):
  """The module in float64 on the host, computed once per shape for all `_SAMPLES` observations (every sample is independent
  of the others, so a test takes the slice it runs): features of both U-Nets and the advantages; left unchanged by the tests."""
  ref = copy.deepcopy(_net(shape)).double().cpu()
  xm, xo = _observations(shape)
  with torch.no_grad():
    x, _ = ref.left(xm.permute(0, 3, 1, 2).double() / 255.0)
    w, _ = ref.right(xo.permute(0, 3, 1, 2).double() / 255.0)
    adv = ref.pos(_xcorr64(x, w)).flatten(1)
  return ref, x, w, adv


def _fast(shape, mode):
  from stackrl_amd import qops
  return qops.FastFeatures(_net(shape), dtype=torch.bfloat16 if mode == _BF16 else torch.float32)


def _inputs(shape, s):
  xm, xo = _observations(shape)
  return xm[s].cuda(), xo[s].cuda()


# Tolerances of the forward, as fractions of the feature scale (the largest |feature| of the float64 reference):
# fp32-class — test_fast_features_fp32_match_the_module's 2e-4;
# bf16 — test_fast_features_match_autocast_features' pair: max 3e-2 and mean 3e-3 against the autocast graph, and a mean error
# against the exact forward of at most 1.5 x the autocast graph's own
_X3_TOL, _BF16_MAX, _BF16_MEAN, _BF16_RATIO = 2e-4, 3e-2, 3e-3, 1.5


@pytest.mark.parametrize('shape,mode,B', FORWARD_CASES, ids=[_case_id(c) for c in FORWARD_CASES])
def test_fast_forward_routes_as_restated_and_matches_float64(shape, mode, B, monkeypatch):
  """`FastFeatures` + `.pos` at B samples: (1) the calls it makes are, layer by layer, the paths tests/rollout_dispatch.py
  restates for (shape, mode, B) — no layer falls to the library, or leaves it, unnoticed; (2) the features against the same
  module in float64 on the host, within the project's bounds for this forward (`_X3_TOL`, or the bf16 pair of conditions);
  (3) the advantages of `.pos` against the float64 head on the same correlation map, within the bounds of
  test_fast_position_head_fp32_tracks_the_module (1e-4 of the range) / test_fast_position_head_tracks_the_module (1e-2).
  The bounds were set at 128 / 32; measured on an MI355X, 64 / 16 sits inside them as 128 / 32 does (fractions of the scale,
  left / right features): fp32-class max 1.0e-5 / 7.2e-6 at 64 / 16 and 1.1e-5 / 1.1e-5 at 128 / 32, the stock float32 module
  6e-7; bf16 against the autocast graph max 2.1e-2 / 1.4e-2 and mean 1.4e-3 / 9.2e-4 at 64 / 16, 2.0e-2 / 2.3e-2 and
  1.5e-3 / 1.4e-3 at 128 / 32; bf16 mean against float64 3.8e-4 / 6.2e-4, the autocast graph's own 1.5e-3 / 1.2e-3.
  The transposed (`nchw`) form of `bias_act` appears in no trace of these modes: both U-Nets end on maps that are whole tiles
  of csrc/conv_mfma.hip, whose own NCHW store writes the features; test_bias_act_is_exact covers that form."""
  from stackrl_amd import qops
  net = _net(shape)
  ref, ex, ew, _ = _reference(shape)
  xm, xo = _inputs(shape, slice(0, B))
  ff = _fast(shape, mode)
  trace = _Trace(monkeypatch)
  with trace.record():
    fx, fw = ff((xm, xo))
    corr = qops.xcorr_forward(fx, fw)
    adv = ff.pos(corr)
  want = D.forward_paths(shape[0], shape[1], mode, B)
  assert trace.paths == want, 'routing differs from the restatement:\n got  {}\n want {}'.format(trace.paths, want)
  assert D.has_library_call(trace.paths) == (not (shape == (128, 32) and mode == _X3 and B == 8))
  if shape == (64, 16) and mode == _BF16:
    assert ('library+bias_act_pool', 'bf16') in trace.paths and ('library+bias_act', 'bf16', 'slice') in trace.paths
  with torch.no_grad():
    sx, _, sw = net.features((xm, xo))                                  # the stock module, float32
    with torch.autocast('cuda', dtype=torch.bfloat16):
      ax, _, aw = net.features((xm, xo))                                # the stock module under bf16 autocast
  for name, got, exact, stock, auto in (('left', fx, ex[:B].cuda(), sx, ax), ('right', fw, ew[:B].cuda(), sw, aw)):
    assert got.shape == exact.shape and got.is_contiguous() and got.dtype == (torch.bfloat16 if mode == _BF16 else torch.float32)
    scale = float(exact.abs().max())
    e_fast = (got.double() - exact).abs()
    e_stock, e_auto = (stock.double() - exact).abs(), (auto.double() - exact).abs()
    d_auto = (got.double() - auto.double()).abs()
    print('{} {} {} B={}: scale {:.4g}; fast vs f64 max {:.3g} mean {:.3g}; stock f32 vs f64 max {:.3g}; autocast vs f64 max {:.3g} mean {:.3g}; '
          'fast vs autocast max {:.3g} mean {:.3g} (fractions of the scale)'.format(
            shape, mode, name, B, scale, float(e_fast.max()) / scale, float(e_fast.mean()) / scale, float(e_stock.max()) / scale,
            float(e_auto.max()) / scale, float(e_auto.mean()) / scale, float(d_auto.max()) / scale, float(d_auto.mean()) / scale))
    if mode == _X3:
      assert float(e_fast.max()) <= _X3_TOL * scale
    else:
      assert float(d_auto.max()) <= _BF16_MAX * scale and float(d_auto.mean()) <= _BF16_MEAN * scale
      assert float(e_fast.mean()) <= _BF16_RATIO * float(e_auto.mean()) + 1e-6 * scale
  with torch.no_grad():
    ra = ref.pos(corr.double().cpu()).flatten(1).cuda()
  assert adv.shape == ra.shape and adv.dtype == torch.float32
  span = float(ra.max() - ra.min())
  print('advantages: max error {:.3g} of the range'.format(float((adv.double() - ra).abs().max()) / span))
  assert float((adv.double() - ra).abs().max()) <= (1e-2 if mode == _BF16 else 1e-4) * span


@pytest.mark.parametrize('shape,mode', INDEPENDENCE_CASES, ids=[_case_id(c) for c in INDEPENDENCE_CASES])
def test_fast_forward_is_position_independent(shape, mode, monkeypatch):
  """The forward of 16 samples against the forwards of its two halves of 8 (every gemm layer takes both batches; at 16 the
  layers whose workgroups take eight maps run two workgroups): features and advantages equal bit for bit where the recorded
  calls hold no library convolution — the hand-written kernels sum in a fixed order whatever the sample's position — and
  within the forward's bounds (`_X3_TOL`; the bf16 max and mean against the other run) where they do."""
  from stackrl_amd import qops
  ff = _fast(shape, mode)
  trace = _Trace(monkeypatch)

  def run(s):
    xm, xo = _inputs(shape, s)
    with trace.record():
      fx, fw = ff((xm, xo))
      adv = ff.pos(qops.xcorr_forward(fx, fw))
    assert trace.paths == D.forward_paths(shape[0], shape[1], mode, xm.shape[0])
    return (fx, fw, adv), D.has_library_call(trace.paths)
  n = INDEPENDENCE_BATCH
  whole, lib = run(slice(0, n))
  assert any(p[0] == 'conv_gemm' and p[3] in (8, 4) and p[-1] == 'multi-wg' for p in trace.paths)
  any_lib = lib
  for s in (slice(0, n // 2), slice(n // 2, n)):
    part, lib = run(s)
    any_lib = any_lib or lib
    for a, b in zip(whole, part):
      if not any_lib:
        assert torch.equal(a[s], b)
      else:
        scale = float(a.float().abs().max())
        d = (a[s].float() - b.float()).abs()
        if mode == _X3:
          assert float(d.max()) <= _X3_TOL * scale
        else:
          assert float(d.max()) <= _BF16_MAX * scale and float(d.mean()) <= _BF16_MEAN * scale
  assert any_lib == (mode == _BF16 or shape == (64, 16))     # 128 / 32 fp32-class: no library call, so the claim above is the exact one


@pytest.mark.parametrize('shape,mode', POLICY_CASES, ids=[_case_id(c) for c in POLICY_CASES])
def test_fused_policy_chunks_pick_float64_maximal_actions(shape, mode):
  """`FusedPolicy` at epsilon 0 over 20 samples in chunks of 8, 8 and 4 and as one call of 20 (`chunk=32`): three routings of
  the same network.  Every action is the other run's, or its float64 advantage is within the mode's tolerance of the float64
  maximum (fp32-class: 2e-4 of the largest |advantage|, the criterion of test_fast_features_fp32_match_the_module; bf16: 2e-2
  of the advantage range, test_fast_position_head_tracks_the_module's)."""
  from stackrl_amd import qops
  net = _net(shape)
  _, _, _, adv = _reference(shape)
  adv = adv.cuda()
  xm, xo = _inputs(shape, slice(0, POLICY_BATCH))
  acts = []
  for chunk in POLICY_CHUNKS:
    pol = qops.FusedPolicy(chunk=chunk, autocast=torch.bfloat16 if mode == _BF16 else None, fast=True)
    draws = qops.FusedPolicy.draws(net, POLICY_BATCH, torch.Generator(device='cuda').manual_seed(1), xm.device)
    acts.append(pol(net, (xm, xo), 0.0, None, draws=draws))
  a, b = acts
  gap = torch.stack([adv.amax(1) - adv.gather(1, t[:, None])[:, 0] for t in acts])
  tol = 2e-4 * adv.abs().amax(1) if mode == _X3 else 2e-2 * (adv.amax(1) - adv.amin(1))
  print('{} {}: {} of {} actions differ between the chunkings; largest gap to the float64 maximum {:.3g} of the tolerance'.format(
    shape, mode, int((a != b).sum()), POLICY_BATCH, float((gap / tol).max())))
  assert int(a.min()) >= 0 and int(b.max()) < net.n_actions
  assert bool(((a == b) | ((gap[0] <= tol) & (gap[1] <= tol))).all())
  if shape == (128, 32) and mode == _X3:
    assert torch.equal(a[:16], b[:16])
