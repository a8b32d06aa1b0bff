"""Every path of csrc/xcorr_mfma.hip held to the float64 result BIT FOR BIT.

The operands (tests/xcorr_cases.py) are chosen so that every product and every partial sum of any order is a float32 value:
the Toeplitz family `k_xcorr_mfma` in its three modes, both geometries, every operand dtype pair and both precisions, with one
channel or several per workgroup and with one channel group or several; the row-product forward `k_xcorr_rows4` at every
channel count its channel groups turn on; `srl_xcorr_rows`; and the autograd function under bf16 features all have to return `xcorr_cases.expect` exactly, and the same bits when run again.  A wrong tap,
column, channel, sample offset, lo plane or rounding shows as a mismatch at a named output element; there is no tolerance to
hide behind.  The one tolerance of the file is the rounding case at the end: dense random float32 operands at precision 0
against the float64 correlation of the operands rounded to bf16, at the project's bound for exact bf16 operands.

The parameter lists are module constants: tests/test_update_dispatch.py (no GPU) imports them and counts the dispatch regimes
they reach."""
import pytest

import xcorr_cases as XC

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

GEOMETRIES = XC.GEOMETRIES
# (B, C): one channel per workgroup; one channel in all (one channel group: no k_sum_partials); two channels per workgroup
# (with the split at 128 / 32 — the only instantiation whose thread count lets PF be true — the next channel is requested
# under the current one's products)
TOEPLITZ_BC = [(3, 16), (3, 1), (32, 16)]
PAIRS = [('f32', 'f32'), ('bf16', 'bf16'), ('f32', 'bf16'), ('bf16', 'f32')]      # (map, kernel) at precision 0
SPLIT_BC = [(3, 16), (32, 16)]                                                      # precision 1
LARGE_BATCH, LARGE_DISTINCT = 256, 5        # one channel group by the batch size: 256 samples cycling through five
ROWS_CHANNELS = [1, 4, 5, 8, 9, 15, 16]     # around `c < C` of the row-product kernel's channel groups (wave + 4 ci, tid / 32 + 8 h)
ROWS_KINDS = ['f32x3', 'f32', 'bf16']       # float32 with the split (split operands), float32 and bf16 at precision 0 (integers)
FOUR_WAVES = '4-%s'                         # case ids name the four-wave kernel, as they did while an eight-wave one ran beside it
ROWS_BATCH = 192                            # the smallest batch that takes the row-product kernel unforced
ROWS_ENTRY_BC = [(1, 5), (1, 16), (3, 5), (3, 16)]
# the rounding case: the forward with two channels per workgroup, the gradients, the row-product kernel
ROUNDING_FORWARD = [(20, 16, 128, 32), (20, 16, 64, 16)]
ROUNDING_GRADIENTS = [(3, 16, 128, 32), (3, 16, 64, 16)]

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}


def assert_exact(got, want, what):
  """`torch.equal`, naming the first elements that differ."""
  want = want.to(got.device)
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
  if not torch.equal(got, want):
    bad = (got != want) | (got != got)
    idx = bad.nonzero()
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:8]]
    raise AssertionError('%s: %d of %d elements differ; first (index, got, want): %s; index ranges %s .. %s'
                         % (what, idx.shape[0], got.numel(), first, idx.min(0).values.tolist(), idx.max(0).values.tolist()))


def device_operands(case, mode):
  """(a, k) of srl_xcorr_mfma for `mode`, float32 on the device, made as `HandNet.backward` makes them: `srl_tcorr_grad` picks
  channel 0 of the position head's input gradient and pads it, `srl_tflip` turns the kernels.  Both are held to the host's
  statement of them, exactly."""
  from stackrl_amd import qops
  x, w = case['x'].cuda(), case['w'].cuda()
  if mode == 0:
    return x, w
  L = qops.load()
  B, C, H, h = case['B'], case['C'], case['H'], case['h']
  O = H - h + 1
  g = case['g_dx' if mode == 1 else 'g_dw']
  gpos = torch.randint(-3, 4, (B, O, O, 16), generator=torch.Generator().manual_seed(B + C)).float()
  gpos[..., 0] = g
  gpos = gpos.cuda()
  gcorr = torch.full((B, O, O), float('nan'), device='cuda')
  gp = torch.full((B, O + 2 * (h - 1), O + 2 * (h - 1)), float('nan'), device='cuda')
  assert L.srl_tcorr_grad(gpos.data_ptr(), 16, gcorr.data_ptr(), gp.data_ptr(), B, O, h - 1, qops._stream(gp)) == 0
  assert_exact(gcorr, g, 'srl_tcorr_grad, gradient')
  assert_exact(gp, XC.pad_gradient(g, h), 'srl_tcorr_grad, padded gradient')
  if mode == 2:
    return x, gcorr
  wflip = torch.full((B, C, h, h), float('nan'), device='cuda')
  assert L.srl_tflip(w.data_ptr(), wflip.data_ptr(), B * C, h * h, qops._stream(gp)) == 0
  assert_exact(wflip, XC.flip(case['w']), 'srl_tflip')
  return gp, wflip


def run_exact(case, mode, precision, dt_a='f32', dt_k='f32', what=''):
  from stackrl_amd import qops
  a, k = device_operands(case, mode)
  a, k = a.to(DT[dt_a]), k.to(DT[dt_k])
  args = (mode, precision, a, k, case['B'], case['C'], case['H'], case['h'])
  got = qops._xcorr_mfma(*args)
  assert_exact(got, XC.expect(case, mode), what)
  assert_exact(qops._xcorr_mfma(*args), got, what + ', run again')
  return got


# ================================================================================================ the Toeplitz kernel
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('dt_a,dt_k', PAIRS)
@pytest.mark.parametrize('B,C', TOEPLITZ_BC)
@pytest.mark.parametrize('H,h', GEOMETRIES)
def test_toeplitz_integer_operands_every_dtype_pair(H, h, B, C, dt_a, dt_k, mode, monkeypatch):
  """Precision 0 on integer operands: float32 operands take `srl_pk_bf16` or `bf16_rne`, bf16 operands the packed loads, the
  mixed pairs what `_XCorrMFMA.backward` launches under bf16 features; the maps of d/dx have odd sides (159 and 79) and are
  staged element by element, by `load_elem<false>` when they are bf16."""
  monkeypatch.setenv('SRL_XCORR_ROWS', '0')
  run_exact(XC.int_case(B, C, H, h), mode, 0, dt_a, dt_k, 'Toeplitz %s x %s mode %d %d/%d B %d C %d' % (dt_a, dt_k, mode, H, h, B, C))


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('B,C', SPLIT_BC)
@pytest.mark.parametrize('H,h', GEOMETRIES)
def test_toeplitz_split_operands(H, h, B, C, mode, monkeypatch):
  """Precision 1: hi hi' + hi lo' + lo hi' with a lo part at every map position and every tap."""
  monkeypatch.setenv('SRL_XCORR_ROWS', '0')
  run_exact(XC.split_case(B, C, H, h), mode, 1, what='Toeplitz bf16x3 mode %d %d/%d B %d C %d' % (mode, H, h, B, C))


def _cycled(case, B):
  """The case's samples repeated in turn up to B samples: (x, w, expected forward) on the device."""
  idx = (torch.arange(B) % case['B']).cuda()
  return case['x'].cuda()[idx], case['w'].cuda()[idx], XC.expect(case, 0).cuda()[idx]


@pytest.mark.parametrize('kind', ROWS_KINDS)
@pytest.mark.parametrize('H,h', GEOMETRIES)
def test_toeplitz_forward_with_one_channel_group(H, h, kind, monkeypatch):
  """256 samples: a workgroup loops over all 16 channels and writes `out` itself — the regime of the 64 / 16 rollout at policy
  chunks of 256 and more.  The samples cycle through five, so `blockIdx.x` alone has to decide the sample."""
  from stackrl_amd import qops
  monkeypatch.setenv('SRL_XCORR_ROWS', '0')
  case = (XC.split_case if kind == 'f32x3' else XC.int_case)(LARGE_DISTINCT, 16, H, h)
  x, w, want = _cycled(case, LARGE_BATCH)
  if kind == 'bf16':
    x, w = x.bfloat16(), w.bfloat16()
  got = qops.xcorr_forward_mfma(x, w, int(kind == 'f32x3'))
  assert_exact(got, want, 'Toeplitz forward %s %d/%d at %d samples' % (kind, H, h, LARGE_BATCH))
  assert_exact(qops.xcorr_forward_mfma(x, w, int(kind == 'f32x3')), got, 'run again')


# ================================================================================================ the row-product kernel
def _rows_operands(kind, B, C):
  case = (XC.split_case if kind == 'f32x3' else XC.int_case)(B, C, 128, 32)
  x, w = case['x'].cuda(), case['w'].cuda()
  if kind == 'bf16':
    x, w = x.bfloat16(), w.bfloat16()
  return case, x, w, int(kind == 'f32x3')


@pytest.mark.parametrize('kind', ROWS_KINDS)
@pytest.mark.parametrize('C', ROWS_CHANNELS, ids=[FOUR_WAVES % C for C in ROWS_CHANNELS])
def test_row_product_kernels_at_every_channel_grouping(C, kind, monkeypatch):
  """`k_xcorr_rows4` (a wave computes channels wave + 4 ci, a thread stages tid / 32 and tid / 32 + 8), forced at 3 samples;
  with integer operands the Toeplitz kernel has to give the same bits."""
  from stackrl_amd import qops
  monkeypatch.setenv('SRL_XCORR_ROWS', '1')
  case, x, w, prec = _rows_operands(kind, 3, C)
  what = 'rows kernel, %s, C %d' % (kind, C)
  got = qops.xcorr_forward_mfma(x, w, prec)
  assert_exact(got, XC.expect(case, 0), what)
  assert_exact(qops.xcorr_forward_mfma(x, w, prec), got, what + ', run again')
  if kind != 'f32x3':
    monkeypatch.setenv('SRL_XCORR_ROWS', '0')
    assert_exact(qops.xcorr_forward_mfma(x, w, prec), got, what + ' against the Toeplitz kernel')


@pytest.mark.parametrize('kind', ROWS_KINDS, ids=[FOUR_WAVES % kind for kind in ROWS_KINDS])
def test_row_product_kernels_chosen_by_the_batch_size(kind, monkeypatch):
  from stackrl_amd import qops
  monkeypatch.delenv('SRL_XCORR_ROWS', raising=False)
  case = (XC.split_case if kind == 'f32x3' else XC.int_case)(LARGE_DISTINCT, 16, 128, 32)
  x, w, want = _cycled(case, ROWS_BATCH)
  if kind == 'bf16':
    x, w = x.bfloat16(), w.bfloat16()
  got = qops.xcorr_forward_mfma(x, w, int(kind == 'f32x3'))
  assert_exact(got, want, 'rows kernel, %s, at %d samples' % (kind, ROWS_BATCH))
  assert_exact(qops.xcorr_forward_mfma(x, w, int(kind == 'f32x3')), got, 'run again')


@pytest.mark.parametrize('kind', ['f32x3', 'bf16'])
@pytest.mark.parametrize('B,C', ROWS_ENTRY_BC)
def test_xcorr_forward_rows_entry(B, C, kind, monkeypatch):
  """`srl_xcorr_rows` behind `qops.xcorr_forward_rows` (greedy acting): float32 operands take the split, bf16 operands are
  used as they are; a sample's map is the same alone and in a batch, which is what the entry is for."""
  from stackrl_amd import qops
  monkeypatch.delenv('SRL_XCORR_ROWS', raising=False)
  case, x, w, _ = _rows_operands(kind, B, C)
  got = qops.xcorr_forward_rows(x, w)
  assert_exact(got, XC.expect(case, 0), 'srl_xcorr_rows %s B %d C %d' % (kind, B, C))
  assert_exact(qops.xcorr_forward_rows(x, w), got, 'run again')
  if B > 1:
    assert_exact(qops.xcorr_forward_rows(x[:1], w[:1]), got[:1], 'sample 0 alone against sample 0 in the batch')


# ================================================================================================ autograd, bf16 features
@pytest.mark.parametrize('H,h', GEOMETRIES)
def test_autograd_under_bf16_features(H, h, monkeypatch):
  """`qops.correlation(qops.BF16)` on bf16 features: the backward launches d/dx with a float32 padded gradient and bf16 flipped
  kernels, d/dw with bf16 maps and a float32 gradient.  The output is float32 and exact.  The two gradients are returned in the
  features' dtype: `_XCorrMFMA.backward` converts the kernels' exact float32 sums to bf16, and sums of 1,024 and 9,409 integer
  products do not all fit bf16's eight bits, so they are held to the exact result ROUNDED TO BF16 (nearest even) — the exact
  float32 sums of the same launches are what test_toeplitz_integer_operands_every_dtype_pair holds."""
  from stackrl_amd import qops
  monkeypatch.setenv('SRL_XCORR_ROWS', '0')
  case = XC.int_case(3, 16, H, h)
  x = case['x'].cuda().bfloat16().requires_grad_()
  w = case['w'].cuda().bfloat16().requires_grad_()
  out = qops.correlation(qops.BF16)(x, w)
  out.backward(case['g_dx'].cuda()[:, None])
  assert_exact(out.detach(), XC.expect(case, 0), 'forward')
  assert x.grad.dtype == w.grad.dtype == torch.bfloat16
  assert_exact(x.grad.float(), XC.expect(case, 1).bfloat16().float(), 'x.grad')
  assert_exact(w.grad.float(), XC.expect(case, 2).bfloat16().float(), 'w.grad')


# ================================================================================================ the rounding of float32 operands
def _rounding(case, mode, got, what):
  rounded, unrounded = XC.rounding_refs(case, mode)
  r, u = XC.ratio(got.cpu(), rounded), XC.ratio(got.cpu(), unrounded)
  print('xcorr rounding: %-44s against bf16(RNE) operands %.3g, against unrounded operands %.3g' % (what, r, u))
  assert r <= XC.ROUNDING_TOL, (what, r)


@pytest.mark.parametrize('B,C,H,h', ROUNDING_FORWARD)
def test_float32_operands_are_rounded_to_nearest_even_forward(B, C, H, h, monkeypatch):
  """Precision 0 on dense random float32 operands against the float64 correlation of the operands rounded to bf16 with RNE, at
  the bound of exact bf16 operands (2e-5 of the scale); against the unrounded operands the same figure is of the order of 1e-3,
  which is why a bound of 6e-3 could not see the rounding mode, a dropped tap or a misplaced element."""
  from stackrl_amd import qops
  monkeypatch.setenv('SRL_XCORR_ROWS', '0')
  case = XC.rounding_case(B, C, H, h)
  _rounding(case, 0, qops.xcorr_forward_mfma(case['x'].cuda(), case['w'].cuda(), 0), 'Toeplitz forward %d/%d B %d' % (H, h, B))


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('B,C,H,h', ROUNDING_GRADIENTS)
def test_float32_operands_are_rounded_to_nearest_even_gradients(B, C, H, h, mode, monkeypatch):
  from stackrl_amd import qops
  monkeypatch.setenv('SRL_XCORR_ROWS', '0')
  case = XC.rounding_case(B, C, H, h)
  a, k = device_operands(case, mode)
  _rounding(case, mode, qops._xcorr_mfma(mode, 0, a, k, B, C, H, h), 'Toeplitz %s %d/%d B %d' % (('', 'd/dx', 'd/dw')[mode], H, h, B))


def test_float32_operands_are_rounded_to_nearest_even_rows(monkeypatch):
  from stackrl_amd import qops
  monkeypatch.setenv('SRL_XCORR_ROWS', '1')
  case = XC.rounding_case(3, 16, 128, 32)
  _rounding(case, 0, qops.xcorr_forward_mfma(case['x'].cuda(), case['w'].cuda(), 0), 'rows kernel B 3')
