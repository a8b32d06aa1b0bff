"""Python side of libstackrl_qnet.so (include/stackrl_qnet.h, stackrl_explore.h, stackrl_greedy.h, stackrl_baseline_rows.h): the one
signature table (`_SIGS`) of the library, its loader (`load`) and checked launch (`call`, both from _bind.py), which qtrain.py
and baselines.py use too, and the hand-written ops of the Q-net rollout path.
No CPU fallback: these functions need a HIP device and the built library."""
import ctypes

import torch

from stackrl_amd import _bind

_VP, _I32, _I64, _F32, _F64, _INT = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_int
# every .hip file keeps the text of its last refusal in a buffer of its own: the accessor that goes with an export is the one
# of the file that defines it (qnet.hip, greedy.hip and heuristics.hip share qnet.hip's)
_QNET, _XCORR, _EPI, _CONV, _GEMM, _LEARN, _TRAIN = ('srl_qnet_last_error', 'srl_xcorr_mfma_last_error', 'srl_epilogue_last_error',
                                                     'srl_conv_last_error', 'srl_conv_gemm_last_error', 'srl_learner_last_error',
                                                     'srl_train_conv_last_error')
# export -> (restype, argtypes, error accessor or None): every declaration of include/stackrl_qnet.h, stackrl_explore.h,
# stackrl_greedy.h and stackrl_baseline_rows.h (pointers as void*); tests/test_abi.py holds the table to the headers and the
# accessors to the sources.  A launching export returns int and takes the stream last; the others are plain queries.
_SIGS = {
  # csrc/qnet.hip, greedy.hip, heuristics.hip
  'srl_xcorr_forward': (_INT, [_VP] * 3 + [_I32] * 6 + [_VP], _QNET),
  'srl_policy_head': (_INT, [_VP] * 3 + [_F32, _VP, _I32, _I32, _VP], _QNET),
  'srl_boltzmann_head': (_INT, [_VP, _VP, _F32, _VP, _I32, _I32, _VP], _QNET),
  'srl_greedy_head': (_INT, [_VP] * 2 + [_I32] * 4 + [_VP] * 4, _QNET),
  'srl_heuristic': (_INT, [_I32] + [_VP] * 4 + [_I32] * 6 + [_F64, _VP], _QNET),
  'srl_baseline_select': (_INT, [_VP, _VP, _I32, _I32, _VP, _VP, _I32, _I32, _VP], _QNET),
  'srl_heuristic_rows': (_INT, [_I32] + [_VP] * 4 + [_I32] * 8 + [_F64, _VP], _QNET),
  'srl_baseline_rows_select': (_INT, [_VP] * 2 + [_I32] * 6 + [_VP] * 4, _QNET),
  'srl_qnet_last_error': (ctypes.c_char_p, [], None),
  'srl_qnet_build_info': (ctypes.c_char_p, [], None),
  # csrc/xcorr_mfma.hip
  'srl_xcorr_mfma_scratch_bytes': (_I64, [_I32] * 6, None),
  'srl_xcorr_mfma': (_INT, [_I32, _I32, _VP, _I32, _VP, _I32, _VP, _VP, _I64] + [_I32] * 4 + [_VP], _XCORR),
  'srl_xcorr_rows': (_INT, [_I32, _VP, _VP, _I32, _VP] + [_I32] * 4 + [_VP], _XCORR),
  'srl_xcorr_mfma_last_error': (ctypes.c_char_p, [], None),
  # csrc/epilogue.hip
  'srl_bias_act': (_INT, [_VP] * 3 + [_I64] + [_I32] * 5 + [_VP], _EPI),
  'srl_bias_act_f32': (_INT, [_VP] * 3 + [_I64] + [_I32] * 5 + [_VP], _EPI),
  'srl_bias_act_pool': (_INT, [_VP] * 4 + [_I32] * 6 + [_VP], _EPI),
  'srl_bias_act_pool_f32': (_INT, [_VP] * 4 + [_I32] * 6 + [_VP], _EPI),
  'srl_bias_act_bwd_scratch_floats': (_I64, [_I64, _I32], None),
  'srl_bias_act_bwd_f32': (_INT, [_VP] * 5 + [_I64, _I32, _I32, _VP], _EPI),
  'srl_pool2x2': (_INT, [_VP] * 2 + [_I32] * 7 + [_VP], _EPI),
  'srl_epilogue_last_error': (ctypes.c_char_p, [], None),
  # csrc/conv_mfma.hip
  'srl_conv3x3_wfrag_elems': (_I32, [_I32] * 2, None),
  'srl_conv3x3_bias_relu': (_INT, [_VP] * 5 + [_I32] * 8 + [_VP], _CONV),
  'srl_conv3x3_bias_relu_f32': (_INT, [_VP] * 5 + [_I32] * 8 + [_VP], _CONV),
  'srl_conv3x3_thin': (_INT, [_VP, _I32, _VP, _VP, _VP] + [_I32] * 6 + [_VP], _CONV),
  'srl_conv3x3_thin_f32': (_INT, [_VP, _I32, _VP, _VP, _VP] + [_I32] * 6 + [_VP], _CONV),
  'srl_conv3x3_relu_project': (_INT, [_VP] * 4 + [_F32, _VP] + [_I32] * 5 + [_VP], _CONV),
  'srl_conv3x3_relu_project_f32': (_INT, [_VP] * 4 + [_F32, _VP] + [_I32] * 5 + [_VP], _CONV),
  'srl_thin_conv3x3_bias_relu_f32': (_INT, [_VP, _I32, _I32] + [_VP] * 6 + [_I32] * 6 + [_VP], _CONV),
  'srl_thin_conv3x3_relu_project_f32': (_INT, [_VP] * 6 + [_F32, _VP] + [_I32] * 3 + [_VP], _CONV),
  'srl_convt2x2_wfrag_elems': (_I32, [_I32] * 2, None),
  'srl_convt2x2_bias_relu': (_INT, [_VP] * 4 + [_I32] * 7 + [_VP], _CONV),
  'srl_convt2x2_bias_relu_f32': (_INT, [_VP] * 4 + [_I32] * 7 + [_VP], _CONV),
  'srl_conv_last_error': (ctypes.c_char_p, [], None),
  # csrc/conv_gemm.hip
  'srl_conv3x3_gemm_supported': (_I32, [_I32] * 3, None),
  'srl_conv3x3_gemm_wfrag_elems': (_I64, [_I32] * 2, None),
  'srl_conv3x3_gemm_batch_multiple': (_I32, [_I32] * 2, None),
  'srl_conv3x3_gemm_bias_relu': (_INT, [_VP] * 4 + [_I32] * 7 + [_VP], _GEMM),
  'srl_convt2x2_gemm_supported': (_I32, [_I32] * 2, None),
  'srl_convt2x2_gemm_bias_relu': (_INT, [_VP] * 4 + [_I32] * 8 + [_VP], _GEMM),
  'srl_conv_gemm_last_error': (ctypes.c_char_p, [], None),
  # csrc/learner.hip
  'srl_td_epilogue': (_INT, [_VP] * 7 + [_F32, _F32, _F32, _I32, _F32, _I32, _I32] + [_VP] * 8, _LEARN),
  'srl_adam_step': (_INT, [_VP] * 4 + [_I64, _VP] + [_F32] * 4 + [_VP], _LEARN),
  'srl_gumbel_topk_scratch_bytes': (_I64, [_I64, _I32], None),
  'srl_gumbel_topk': (_INT, [_VP] * 3 + [_I64, _I32] + [_VP] * 3 + [_I64, _VP], _LEARN),
  'srl_replay_scatter': (_INT, [_VP, _VP, _I64, _I64, _VP, _VP, _VP, _I32, _I64, _I64] + [_VP] * 7, _LEARN),
  'srl_replay_gather': (_INT, [_VP, _I32, _I64, _I64, _I32, _VP, _VP, _VP, _I64, _I64] + [_VP] * 16, _LEARN),
  'srl_logit_extrema_scratch_bytes': (_I64, [], None),
  'srl_logit_extrema': (_INT, [_VP, _I64] + [_VP] * 4, _LEARN),
  'srl_learner_last_error': (ctypes.c_char_p, [], None),
  # csrc/train_conv.hip
  'srl_tconv': (_INT, [_VP, _I32, _I32, _VP, _VP, _VP] + [_I32] * 10 + [_VP], _TRAIN),
  'srl_twrw_scratch_floats': (_I64, [_I32] * 6, None),
  'srl_twrw': (_INT, [_VP, _I32, _I32, _VP, _VP, _VP] + [_I32] * 7 + [_VP, _I32, _I32, _VP, _VP], _TRAIN),
  'srl_tact_bwd_scratch_floats': (_I64, [_I64, _I32], None),
  'srl_tact_bwd_blocks': (_I32, [_I64, _I32], None),
  'srl_tact_bwd': (_INT, [_VP, _I32, _I32, _VP, _I32, _I32] + [_VP] * 4 + [_I32] * 6 + [_VP], _TRAIN),
  'srl_trepack': (_INT, [_VP, _VP, _VP, _I32, _I64, _VP], _TRAIN),
  'srl_thead_fwd': (_INT, [_VP] * 5 + [_I32, _I32, _VP], _TRAIN),
  'srl_thead_bwd': (_INT, [_VP] * 8 + [_I32, _I32, _VP], _TRAIN),
  'srl_tvalue_fwd': (_INT, [_VP] * 8 + [_I32] * 4 + [_VP], _TRAIN),
  'srl_tvalue_bwd': (_INT, [_VP] * 12 + [_I32] * 4 + [_VP], _TRAIN),
  'srl_tlayout': (_INT, [_VP, _I32, _I32, _VP] + [_I32] * 4 + [_VP], _TRAIN),
  'srl_tcorr_grad': (_INT, [_VP, _I32, _VP, _VP, _I32, _I32, _I32, _VP], _TRAIN),
  'srl_tflip': (_INT, [_VP, _VP, _I64, _I32, _VP], _TRAIN),
  'srl_tu8_to_f32': (_INT, [_VP, _VP, _I64, _VP], _TRAIN),
  'srl_train_conv_last_error': (ctypes.c_char_p, [], None),
}


load, call = _bind.binding('qnet', _SIGS)
_stream = _bind.stream


_SCRATCH = {}
MFMA_SHAPES = ((128, 32), (64, 16))   # forward (H, kh) shapes built in csrc/xcorr_mfma.hip
BF16, BF16X3 = 0, 1                   # precisions of the MFMA path (include/stackrl_qnet.h)


def _xcorr_mfma(mode, precision, a, k, B, C, H, kh):
  """One launch of srl_xcorr_mfma (see the header for the three modes).  a / k: contiguous bf16 or fp32 tensors."""
  if not a.is_cuda:
    raise RuntimeError('the MFMA cross-correlation needs a HIP device (no CPU fallback)')
  if precision == BF16X3:
    a = a.float(); k = k.float()
  a = a.contiguous(); k = k.contiguous()
  for t in (a, k):
    if t.dtype not in (torch.float32, torch.bfloat16):
      raise TypeError('xcorr operands must be float32 or bfloat16')
  L = load()
  need = L.srl_xcorr_mfma_scratch_bytes(mode, precision, B, C, H, kh)
  if need < 0:
    raise RuntimeError('MFMA cross-correlation: unsupported shape (H=%d, kh=%d)' % (H, kh))
  key = (a.device.index, torch.cuda.current_stream(a.device).cuda_stream)
  scratch = _SCRATCH.get(key)
  if scratch is None or scratch.numel() < need:
    scratch = torch.empty(need, dtype=torch.uint8, device=a.device)
    _SCRATCH[key] = scratch
  O = H - kh + 1
  shape = {0: (B, 1, O, O), 1: (B, C, H, H), 2: (B, C, kh, kh)}[mode]
  out = torch.empty(shape, dtype=torch.float32, device=a.device)
  call('srl_xcorr_mfma', a, mode, precision, a, int(a.dtype == torch.float32), k, int(k.dtype == torch.float32), out, scratch,
       scratch.numel(), B, C, H, kh)
  return out


def _mfma_ok(x, w):
  return x.dim() == 4 and x.shape[-1] == x.shape[-2] and w.shape[-1] == w.shape[-2] and \
         (x.shape[-1], w.shape[-1]) in MFMA_SHAPES


def xcorr_forward_mfma(x, w, precision=BF16):
  """`layers.correlation` forward on the matrix cores: x [B,C,H,H], w [B,C,kh,kh] -> float32 [B,1,OH,OW]."""
  B, C, H, _ = x.shape
  return _xcorr_mfma(0, precision, x, w, B, C, H, w.shape[-1])


class _XCorrMFMA(torch.autograd.Function):
  """Differentiable `layers.correlation` (layers.py:21-38) on the matrix cores: forward and both gradients are the
  same Toeplitz-MFMA kernel family (csrc/xcorr_mfma.hip)."""

  @staticmethod
  def forward(ctx, x, w, precision):
    ctx.save_for_backward(x, w)
    ctx.precision = precision
    return xcorr_forward_mfma(x, w, precision)

  @staticmethod
  def backward(ctx, g):
    x, w = ctx.saved_tensors
    B, C, H, _ = x.shape
    kh = w.shape[-1]
    g = g[:, 0].float()
    dx = dw = None
    if ctx.needs_input_grad[0]:
      gp = torch.nn.functional.pad(g, (kh - 1, kh - 1, kh - 1, kh - 1))
      dx = _xcorr_mfma(1, ctx.precision, gp, w.flip(-1, -2), B, C, H, kh).to(x.dtype)
    if ctx.needs_input_grad[1]:
      dw = _xcorr_mfma(2, ctx.precision, x, g, B, C, H, kh).to(w.dtype)
    return dx, dw, None


def correlation(precision=BF16X3):
  """A drop-in for `nets.correlation_reference` (assign to `net.correlation`): MFMA kernels for the shapes in
  MFMA_SHAPES on a HIP device, the library formulation otherwise."""
  from stackrl_amd import nets

  def f(x, w):
    if x.is_cuda and _mfma_ok(x, w):
      return _XCorrMFMA.apply(x, w, precision)
    return nets.correlation_reference(x, w)
  return f


def xcorr_forward(x, w, precision=None):
  """`layers.correlation` forward (layers.py:21-38): x [B,C,H,W], w [B,C,kh,kw] -> float32 [B,1,OH,OW].
  For the shapes in MFMA_SHAPES the matrix-core kernel runs: bfloat16 features (the autocast rollout path) with
  operands as they are, float32 features with the hi/lo split (bf16x3: fp32-class accuracy, same stated tolerance as
  the vector kernel).  Other shapes, or precision='fp32', take the fp32 vector kernel."""
  if not x.is_cuda:
    raise RuntimeError('xcorr_forward needs a HIP device (no CPU fallback)')
  if precision != 'fp32' and _mfma_ok(x, w):
    if x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16:
      return xcorr_forward_mfma(x, w, BF16)
    if x.dtype == torch.float32 and w.dtype == torch.float32:
      return xcorr_forward_mfma(x, w, BF16X3)
  x = x.contiguous().float(); w = w.contiguous().float()
  B, C, H, W = x.shape
  kh, kw = w.shape[-2:]
  out = torch.empty((B, 1, H - kh + 1, W - kw + 1), dtype=torch.float32, device=x.device)
  call('srl_xcorr_forward', x, x, w, out, B, C, H, W, kh, kw)
  return out


def xcorr_forward_rows(x, w):
  """`xcorr_forward` for greedy acting: where the row-product kernel is built (128 / 32 maps of at most 16 channels, both
  operands float32 — hi / lo split — or both bfloat16) it runs at any batch size (include/stackrl_greedy.h srl_xcorr_rows), so
  a sample's map does not depend on the batch it is evaluated in; other shapes take `xcorr_forward`."""
  if not (x.is_cuda and x.dim() == 4 and tuple(x.shape[-2:]) == (128, 128) and tuple(w.shape[-2:]) == (32, 32) and x.shape[1] <= 16 and
          x.dtype == w.dtype and x.dtype in (torch.float32, torch.bfloat16)):
    return xcorr_forward(x, w)
  x = x.contiguous(); w = w.contiguous()
  B, C = x.shape[:2]
  f32 = int(x.dtype == torch.float32)
  out = torch.empty((B, 1, 97, 97), dtype=torch.float32, device=x.device)
  call('srl_xcorr_rows', x, BF16X3 if f32 else BF16, x, w, f32, out, B, C, 128, 32)
  return out


def policy_head(adv, u, rnd, epsilon):
  """Epsilon-greedy head (dqn.py:334-348): adv [B,A] f32, u [B] f32, rnd [B] i64 -> actions [B] i64."""
  adv = adv.contiguous().float()
  B, A = adv.shape
  actions = torch.empty(B, dtype=torch.int64, device=adv.device)
  call('srl_policy_head', adv, adv, u.contiguous(), rnd.contiguous(), float(epsilon), actions, B, A)
  return actions


def boltzmann_head(adv, keys, temperature):
  """Boltzmann head (dqn.py:349-358; the noise definition: include/stackrl_explore.h): adv [B,A] f32, keys [B,2] i64 (one
  Philox stream key per sample, two 32-bit words) -> actions [B] i64."""
  if not adv.is_cuda:
    raise RuntimeError('boltzmann_head needs a HIP device (no CPU fallback)')
  adv = adv.contiguous().float()
  B, A = adv.shape
  if keys.dtype != torch.int64 or tuple(keys.shape) != (B, 2) or keys.device != adv.device:
    raise ValueError('keys must be an int64 [{}, 2] tensor on {}'.format(B, adv.device))
  actions = torch.empty(B, dtype=torch.int64, device=adv.device)
  call('srl_boltzmann_head', adv, adv, keys.contiguous(), float(temperature), actions, B, A)
  return actions


def greedy_head(adv, v=None, n_valid=None, stats=False, values=False):
  """Greedy head (the definition: include/stackrl_greedy.h): adv [B,A] or [B,G,A] f32 (G rows per env, the first `n_valid`
  valid; None = all), v [B] f32 or None (not dueling: q = adv) -> actions [B] i64 (the flat index r * A + p), then, as asked,
  stats [B,4] f64 {max q, min q, sum q, sum q^2} and q (float32, the shape of adv; rows beyond n_valid are -inf)."""
  if not adv.is_cuda:
    raise RuntimeError('greedy_head needs a HIP device (no CPU fallback)')
  if adv.dim() not in (2, 3):
    raise ValueError('greedy_head: adv must be [B, A] or [B, G, A], got {}'.format(tuple(adv.shape)))
  adv = adv.contiguous().float()
  B, G, A = (adv.shape[0], 1, adv.shape[1]) if adv.dim() == 2 else adv.shape
  if v is not None:
    if v.numel() != B or v.device != adv.device:
      raise ValueError('greedy_head (srl_greedy_head): v must hold {} values on {}, got {} on {}'.format(B, adv.device, tuple(v.shape), v.device))
    v = v.reshape(B).contiguous().float()
  n_valid = G if n_valid is None else int(n_valid)
  actions = torch.empty(B, dtype=torch.int64, device=adv.device)
  st = torch.empty((B, 4), dtype=torch.float64, device=adv.device) if stats else None
  q = torch.empty_like(adv) if values else None
  call('srl_greedy_head', adv, adv, v, B, G, n_valid, A, actions, st, q)
  out = (actions,) + ((st,) if stats else ()) + ((q,) if values else ())
  return out if len(out) > 1 else actions


_CL = torch.channels_last


def _cl(t):
  return t if t.is_contiguous(memory_format=_CL) else t.contiguous(memory_format=_CL)


def bias_act(y, bias, out=None, out_offset=0, relu=True, nchw=False):
  """relu(y + bias[c]) in one pass (csrc/epilogue.hip).  y: bf16 or float32 [B,C,H,W] channels-last.  out: None = in
  place; a channels-last tensor of the same dtype with >= C channels = write into its channel slice
  [out_offset, out_offset + C); nchw=True returns a new NCHW-contiguous tensor (the layout the cross-correlation kernel
  reads)."""
  B, C, H, W = y.shape
  if nchw:
    dst = torch.empty((B, C, H, W), dtype=y.dtype, device=y.device)
    stride, hw = C, H * W
  else:
    dst = y if out is None else out
    stride, hw = dst.shape[1], 0
  call('srl_bias_act_f32' if y.dtype == torch.float32 else 'srl_bias_act', y, y, dst, bias, B * H * W, C, stride, out_offset, hw, int(relu))
  return dst


class _BiasAct(torch.autograd.Function):
  """y <- relu(y + bias) in place on the convolution's output, with the hand-written backward (csrc/epilogue.hip
  k_bias_act_bwd): gx = gy * (y > 0) and the bias gradient summed in a fixed order, one pass over gy and y."""

  @staticmethod
  def forward(ctx, y, bias, relu):
    bias_act(y, bias, relu=relu)
    ctx.mark_dirty(y)
    ctx.relu = bool(relu)
    ctx.save_for_backward(y)
    return y

  @staticmethod
  def backward(ctx, gy):
    y, = ctx.saved_tensors
    B, C, H, W = y.shape
    gy = gy.contiguous(memory_format=_CL)
    gx = torch.empty_like(gy, memory_format=_CL)
    gb = torch.empty(C, dtype=torch.float32, device=y.device)
    scratch = torch.empty(load().srl_bias_act_bwd_scratch_floats(B * H * W, C), dtype=torch.float32, device=y.device)
    call('srl_bias_act_bwd_f32', y, gy, y, gx, gb, scratch, B * H * W, C, int(ctx.relu))
    return gx, gb, None


def bias_act_supported(channels):
  return channels % 8 == 0 and channels <= 256 and 256 % (channels // 8) == 0


def bias_act_autograd(y, bias, relu=True):
  """relu(y + bias[c]) (or y + bias[c]) of a float32 convolution output [B,C,H,W], differentiable: in place on y (made
  channels-last), forward and backward by the kernels of csrc/epilogue.hip.  The update path's replacement for the
  library's separate bias add, ReLU, ReLU backward and bias-gradient reduction."""
  if y.dtype != torch.float32 or not y.is_cuda:
    raise RuntimeError('bias_act_autograd: float32 CUDA tensors only')
  y = y.contiguous(memory_format=_CL)
  if not (torch.is_grad_enabled() and (y.requires_grad or bias.requires_grad)):
    return bias_act(y, bias.detach(), relu=relu)
  return _BiasAct.apply(y, bias, relu)


def bias_act_pool(y, bias, skip, skip_offset):
  """relu(y + bias[c]) into the channel slice [skip_offset, skip_offset + C) of `skip`, plus its 2 x 2 max-pool."""
  B, C, H, W = y.shape
  pooled = torch.empty((B, C, H // 2, W // 2), dtype=y.dtype, device=y.device, memory_format=_CL)
  call('srl_bias_act_pool_f32' if y.dtype == torch.float32 else 'srl_bias_act_pool', y, y, skip, pooled, bias, B, H, W, C, skip.shape[1],
       skip_offset)
  return pooled


def pool2x2(buf, C, offset=0):
  """2 x 2 max-pool of the channel slice [offset, offset + C) of a channels-last bf16 / float32 buffer [B,Ctot,H,W]."""
  B, Ct, H, W = buf.shape
  pooled = torch.empty((B, C, H // 2, W // 2), dtype=buf.dtype, device=buf.device, memory_format=_CL)
  call('srl_pool2x2', buf, buf, pooled, B, H, W, C, Ct, offset, int(buf.dtype == torch.float32))
  return pooled


_PACK_INDEX = {}


def _pack(w, kind, build, x3=False):
  """Gather of a weight tensor into a kernel's fragment order.  The flat gather index (and the mask of padded taps)
  depends on the layer shape only and is built once per (kind, shape, device): re-packing after every weight update —
  once per rollout while training — is then one gather per layer.  x3: the fragments of bf16(w), then those of
  bf16(w - bf16(w)) (the fp32-class kernels)."""
  key = (kind, tuple(w.shape), w.device)
  if key not in _PACK_INDEX:
    _PACK_INDEX[key] = build()
  idx, mask = _PACK_INDEX[key]
  flat = w.detach().float().reshape(-1)
  if x3:
    hi = flat.to(torch.bfloat16)
    lo = (flat - hi.float()).to(torch.bfloat16)
    out = torch.cat([hi[idx], lo[idx]])
    return out * torch.cat([mask, mask]) if mask is not None else out
  out = flat.to(torch.bfloat16)[idx]
  return out * mask if mask is not None else out


def _conv3x3_index(cout, cin, dev):
  ks = torch.arange(5 if cin == 16 else 9 * (cin // 32), device=dev)[:, None, None, None]
  mt = torch.arange(cout // 16, device=dev)[None, :, None, None]
  lane = torch.arange(64, device=dev)[None, None, :, None]
  j = torch.arange(8, device=dev)[None, None, None, :]
  k = 8 * (lane >> 4) + j
  if cin == 16:
    tap, ci = 2 * ks + (k >> 4), k & 15
  else:
    m = cin // 32
    tap, ci = ks // m + 0 * k, 32 * (ks % m) + k
  co = 16 * mt + (lane & 15)
  tapc = tap.clamp(max=8)
  idx = ((co * cin + ci) * 9 + tapc).reshape(-1)
  mask = (tap < 9).expand_as(idx.reshape(tapc.shape[0], co.shape[1], 64, 8)).reshape(-1).to(torch.bfloat16) if cin == 16 else None
  return idx, mask


def pack_conv3x3_weights(w, x3=False):
  """Conv2d weight [cout, cin, 3, 3] -> bf16 A-fragment order of csrc/conv_mfma.hip (see include/stackrl_qnet.h)."""
  cout, cin = int(w.shape[0]), int(w.shape[1])
  n = load().srl_conv3x3_wfrag_elems(cin, cout)
  if n < 0:
    raise ValueError('conv3x3 MFMA kernel: unsupported channels %d -> %d' % (cin, cout))
  out = _pack(w, 'conv3x3', lambda: _conv3x3_index(cout, cin, w.device), x3)
  assert out.numel() == n * (2 if x3 else 1)
  return out


def pack_conv3x3_weights_x3(w):
  """Conv2d weight [cout, cin, 3, 3] (cin in {16, 32, 64}, cout in {16, 32}) -> the two bf16 fragment sets of the fp32-class kernel
  (srl_conv3x3_bias_relu_f32): the fragments of bf16(w), then those of bf16(w - bf16(w))."""
  return pack_conv3x3_weights(w, x3=True)


def conv3x3_bias_relu(x, wfrag, bias, cout, out=None, out_offset=0, pool=False, nchw=False):
  """relu(conv3x3(x) + bias) on the matrix cores (csrc/conv_mfma.hip).  x: bf16 [B,cin,H,W] channels-last.  Returns
  the output (a new channels-last tensor, or `out` whose channel slice [out_offset, out_offset + cout) was written, or
  an NCHW-contiguous tensor with nchw=True) and, with pool=True, also the 2 x 2 max-pooled tensor."""
  B, cin, H, W = x.shape
  if nchw:
    dst = torch.empty((B, cout, H, W), dtype=x.dtype, device=x.device)
    stride = cout
  else:
    dst = out if out is not None else torch.empty((B, cout, H, W), dtype=x.dtype, device=x.device, memory_format=_CL)
    stride = dst.shape[1]
  pooled = torch.empty((B, cout, H // 2, W // 2), dtype=x.dtype, device=x.device, memory_format=_CL) if pool else None
  # float32 tensors take the fp32-class kernel (bf16x3 products, wfrag from pack_conv3x3_weights_x3)
  call('srl_conv3x3_bias_relu_f32' if x.dtype == torch.float32 else 'srl_conv3x3_bias_relu', x, x, wfrag, bias, dst, pooled, B, H, W, cin,
       cout, stride, out_offset, int(nchw))
  return (dst, pooled) if pool else dst


def _conv3x3_gemm_index(cout, cin, dev):
  cb = torch.arange(cin // 32, device=dev)[:, None, None, None, None]
  tap = torch.arange(9, device=dev)[None, :, None, None, None]
  mt = torch.arange(cout // 16, device=dev)[None, None, :, None, None]
  lane = torch.arange(64, device=dev)[None, None, None, :, None]
  j = torch.arange(8, device=dev)[None, None, None, None, :]
  co, ci = 16 * mt + (lane & 15), 32 * cb + 8 * (lane >> 4) + j
  return ((co * cin + ci) * 9 + tap).reshape(-1), None


def pack_conv3x3_gemm_weights(w, x3=False):
  """Conv2d weight [cout, cin, 3, 3] -> bf16 A-fragment order of csrc/conv_gemm.hip ([cin / 32][tap][cout / 16][lane][8]);
  x3: the fragments of bf16(w) followed by those of bf16(w - bf16(w)) (the fp32-class kernel)."""
  cout, cin = int(w.shape[0]), int(w.shape[1])
  out = _pack(w, 'conv3x3_gemm', lambda: _conv3x3_gemm_index(cout, cin, w.device), x3)
  assert out.numel() == load().srl_conv3x3_gemm_wfrag_elems(cin, cout) * (2 if x3 else 1)
  return out


def conv3x3_gemm_supported(cin, cout, W, B):
  L = load()
  return bool(L.srl_conv3x3_gemm_supported(cin, cout, W)) and B % L.srl_conv3x3_gemm_batch_multiple(cout, W) == 0


def conv3x3_gemm_bias_relu(x, wfrag, bias, cout, out=None, out_offset=0):
  """relu(conv3x3(x) + bias) of a deep U-Net level as an implicit GEMM on the matrix cores (csrc/conv_gemm.hip).
  x: bf16 or float32 (fp32-class products, wfrag packed with x3=True) [B,cin,W,W] channels-last; returns a new
  channels-last tensor or `out` whose channel slice [out_offset, out_offset + cout) was written."""
  B, cin, H, W = x.shape
  assert H == W
  dst = out if out is not None else torch.empty((B, cout, H, W), dtype=x.dtype, device=x.device, memory_format=_CL)
  call('srl_conv3x3_gemm_bias_relu', x, x, wfrag, bias, dst, B, W, cin, cout, dst.shape[1], out_offset, int(x.dtype == torch.float32))
  return dst


def _convt2x2_index(cin, cout, dev):
  ks = torch.arange(cin // 32, device=dev)[:, None, None, None]
  mt = torch.arange(4 * cout // 16, device=dev)[None, :, None, None]
  lane = torch.arange(64, device=dev)[None, None, :, None]
  j = torch.arange(8, device=dev)[None, None, None, :]
  ci = 32 * ks + 8 * (lane >> 4) + j
  m = 16 * mt + (lane & 15)
  q, co = m // cout, m % cout
  return ((ci * cout + co) * 4 + q).reshape(-1), None     # w[ci][co][q >> 1][q & 1]


def pack_convt2x2_weights(w, x3=False):
  """ConvTranspose2d weight [cin, cout, 2, 2] -> bf16 A-fragment order of k_convt2x2 (include/stackrl_qnet.h)."""
  cin, cout = int(w.shape[0]), int(w.shape[1])
  n = load().srl_convt2x2_wfrag_elems(cin, cout)
  if n < 0:
    raise ValueError('convT 2x2 MFMA kernel: unsupported channels %d -> %d' % (cin, cout))
  out = _pack(w, 'convt2x2', lambda: _convt2x2_index(cin, cout, w.device), x3)
  assert out.numel() == n * (2 if x3 else 1)
  return out


def pack_convt2x2_weights_x3(w):
  """ConvTranspose2d weight -> the hi and lo bf16 fragment sets of the fp32-class kernel (srl_convt2x2_bias_relu_f32)."""
  return pack_convt2x2_weights(w, x3=True)


def convt2x2_gemm_bias_relu(x, wfrag, bias, cout, out, out_offset=0):
  """relu(conv_transpose2d(x, k=2, s=2) + bias) of the deep levels (128 -> 64, 256 -> 128; any map size) into the channel
  slice of `out`, csrc/conv_gemm.hip k_convt2x2_gemm; bf16 or float32 (wfrag from pack_convt2x2_weights(w, x3=True))."""
  B, cin, H, W = x.shape
  call('srl_convt2x2_gemm_bias_relu', x, x, wfrag, bias, out, B, H, W, cin, cout, out.shape[1], out_offset, int(x.dtype == torch.float32))
  return out


def convt2x2_bias_relu(x, wfrag, bias, cout, out, out_offset=0):
  """relu(conv_transpose2d(x, k=2, s=2) + bias) into the channel slice [out_offset, out_offset + cout) of `out`
  (channels-last, twice the spatial size of x), csrc/conv_mfma.hip.  bf16 tensors: bf16 MFMA; float32 tensors: the
  fp32-class kernel (wfrag from pack_convt2x2_weights_x3)."""
  B, cin, H, W = x.shape
  call('srl_convt2x2_bias_relu_f32' if x.dtype == torch.float32 else 'srl_convt2x2_bias_relu', x, x, wfrag, bias, out, B, H, W, cin, cout,
       out.shape[1], out_offset)
  return out


def pack_thin_weights(w):
  """Conv2d weight [16, cin, 3, 3] (cin 1 or 2) -> float32 [16, 3, 3, cin], the order the thin-layer kernels read."""
  return w.detach().float().permute(0, 2, 3, 1).contiguous()


def conv3x3_thin(x, w, bias, out=None, dtype=torch.bfloat16):
  """relu(conv3x3(x) + bias) for 1 or 2 input channels -> 16 (csrc/conv_mfma.hip, vector ALU).  x: uint8 (scaled by
  1/255) or float32, channels-last memory [B,H,W,cin]; w from `pack_thin_weights`.  Returns bf16 (or float32, per `dtype` / `out`) [B,16,Hp,Wp]
  channels-last; `out` (optional) is a larger zero-margined buffer of that kind whose top-left H x W region is written."""
  B, H, W, cin = x.shape
  if out is None:
    out = torch.empty((B, 16, H, W), dtype=dtype, device=x.device, memory_format=_CL)
  call('srl_conv3x3_thin_f32' if out.dtype == torch.float32 else 'srl_conv3x3_thin', x, x, int(x.dtype != torch.uint8), w, bias, out,
       B, H, W, cin, out.shape[2], out.shape[3])
  return out


def conv3x3_relu_project(x, wfrag, bias, proj_w, proj_b, hv, wv):
  """sum_c proj_w[c] relu(conv3x3(x)[c] + bias[c]) + proj_b, float32 [B,hv,wv]: the last two layers of `pos_layers`."""
  B, _, H, W = x.shape
  out = torch.empty((B, hv, wv), dtype=torch.float32, device=x.device)
  call('srl_conv3x3_relu_project_f32' if x.dtype == torch.float32 else 'srl_conv3x3_relu_project', x, x, wfrag, bias, proj_w, float(proj_b),
       out, B, H, W, hv, wv)
  return out


def thin_conv3x3_bias_relu(x, w1, b1, wfrag, bias, out=None, out_offset=0, pool=False, nchw=False):
  """`conv3x3_thin` (float32 output) followed by `conv3x3_bias_relu` (16 -> 16, fp32-class) as one kernel: the 16-channel
  intermediate stays in LDS.  x: uint8 or float32 [B,H,W,cin] (cin 1 or 2; H, W multiples of 16), w1 from
  `pack_thin_weights`; returns what
  `conv3x3_bias_relu` returns, equal bit for bit."""
  B, H, W, cin = x.shape
  if nchw:
    dst = torch.empty((B, 16, H, W), dtype=torch.float32, device=x.device)
    stride = 16
  else:
    dst = out if out is not None else torch.empty((B, 16, H, W), dtype=torch.float32, device=x.device, memory_format=_CL)
    stride = dst.shape[1]
  pooled = torch.empty((B, 16, H // 2, W // 2), dtype=torch.float32, device=x.device, memory_format=_CL) if pool else None
  call('srl_thin_conv3x3_bias_relu_f32', x, x, int(x.dtype != torch.uint8), cin, w1, b1, wfrag, bias, dst, pooled, B, H, W, stride,
       out_offset, int(nchw))
  return (dst, pooled) if pool else dst


def thin_conv3x3_relu_project(x, w1, b1, wfrag, bias, proj_w, proj_b):
  """`pos_layers` whole as one kernel (fp32-class): x float32 [B,H,W] -> float32 [B,H,W]; equal bit for bit to
  `conv3x3_thin` into a zero-margined map followed by `conv3x3_relu_project`."""
  B, H, W = x.shape
  out = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
  call('srl_thin_conv3x3_relu_project_f32', x, x, w1, b1, wfrag, bias, proj_w, float(proj_b), out, B, H, W)
  return out


class _LazyPacked(object):
  """Packed weights by module: `m in d` = the module has a hand-written kernel; `d[m]` packs on first use after a weight
  update (a layer whose kernel is not used at the current map size is never packed)."""

  def __init__(self):
    self._make = {}
    self._done = {}

  def offer(self, m, make):
    self._make[m] = make

  def __contains__(self, m):
    return m in self._make

  def __getitem__(self, m):
    if m not in self._done:
      self._done[m] = self._make[m]()
    return self._done[m]

  def packed(self):
    """(module, packed weights) of what has been packed since the last weight update."""
    return list(self._done.items())


class _WeightBias(object):
  """(weight in the forward's dtype and channels-last, float32 bias) of a module; the weight copy is made on first use."""

  def __init__(self, m, dtype):
    self._m, self._dtype, self._w = m, dtype, None
    self._b = m.bias.detach().float().contiguous()

  def __getitem__(self, i):
    if i == 1:
      return self._b
    if i != 0:
      raise IndexError(i)
    if self._w is None:
      self._w = self._m.weight.detach().to(self._dtype).contiguous(memory_format=_CL)
    return self._w

  def __iter__(self):
    return iter((self[0], self[1]))


class FastFeatures(object):
  """Inference-only forward of the two U-Nets (`DeepQSiamFCN.features`, models.py:160-177; `layers.unet`,
  layers.py:135-259) in bf16 channels-last: library convolutions without bias, and the fused element-wise passes of
  csrc/epilogue.hip instead of separate bias / ReLU / max-pool / concatenate / layout kernels.  Returns the left and
  right feature maps NCHW-contiguous, ready for the MFMA cross-correlation."""

  def __init__(self, net, mfma_conv=True, dtype=torch.bfloat16, x3_conv=True, fuse_thin=True):
    self.net = net
    self.fuse_thin = bool(fuse_thin)   # fp32-class: thin layer + the 16 -> 16 layer behind it as one kernel (False: two, same values)
    # dtype float32 = the reference's dtype: (x3_conv) the same hand-written layers as the bf16 mode, in fp32-class
    # precision — the 16- / 32-output-channel 3 x 3 layers, the 32 -> 16 / 64 -> 32 transposed convolutions and the
    # position head with bf16x3 products on the matrix cores (csrc/conv_mfma.hip k_conv3x3_x3, k_convt2x2_x3), the thin
    # first layers in fp32 on the vector ALU; the >= 64-output-channel layers are library fp32 convolutions without bias
    # + the fused fp32 epilogues
    self.dtype = dtype
    self.mfma_conv = bool(mfma_conv) and dtype == torch.bfloat16   # hand-written MFMA kernel for the 16- / 32-channel 3 x 3 layers
    self.x3_conv = bool(x3_conv) and dtype == torch.float32
    self._key = None
    self._w = {}
    self._wf = _LazyPacked()
    self._wt = {}
    self._wg = _LazyPacked()
    self._w1 = _LazyPacked()
    self._pos = None
    self._posbuf = {}

  def _refresh(self):
    # `_weights_epoch` is bumped by whoever updates the parameters outside ATen's sight: a hipGraph replay of the
    # optimiser step (DQN._run_segment) changes the weights without touching any tensor's version counter
    key = tuple(p._version for p in self.net.parameters()) + (id(self.net), getattr(self.net, '_weights_epoch', 0))
    if key == self._key:
      return
    self._w = {}
    self._wf = _LazyPacked()
    self._wt = {}
    self._wg = _LazyPacked()
    self._w1 = _LazyPacked()        # transposed convolutions left to the float32 1 x 1 form of the update's kernel (srl_tconv)
    packers = {'conv_mfma': (self._wf, pack_conv3x3_weights), 'gemm': (self._wg, pack_conv3x3_gemm_weights),
               'convt_mfma': (self._wf, pack_convt2x2_weights), 'convt_gemm': (self._wg, pack_convt2x2_weights)}
    for m in self.net.modules():
      if not isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
        continue
      self._w[m] = _WeightBias(m, self.dtype)
      family = self._family(m)
      if family == 'thin':
        self._wt[m] = pack_thin_weights(m.weight)
      elif family in packers:
        store, pack = packers[family]
        store.offer(m, lambda m=m, pack=pack: pack(m.weight, x3=self.x3_conv))
      # weights [cin][q cout + co], q = 2 dy + dx.  A convt_mfma layer keeps this form beside its own: that kernel wants rows of
      # whole 16-pixel tiles (the right U-Net's 64 -> 32 at 8 x 8 has none); convt_gemm takes any map size and needs no second form
      if family == 'tconv' or (family == 'convt_mfma' and self._tconv_ok(m)):
        self._w1.offer(m, lambda m=m: m.weight.detach().float().permute(0, 2, 3, 1).reshape(m.in_channels, 4 * m.out_channels).contiguous())
    pos = getattr(self.net, 'pos', None)
    self._pos = None
    if (self.mfma_conv or self.x3_conv) and pos is not None and len(pos) == 5 and pos[0] in self._wt and pos[2] in self._wf and \
       pos[4].kernel_size == (1, 1) and pos[4].in_channels == 16 and pos[4].out_channels == 1:
      self._pos = (pos[4].weight.detach().float().reshape(16).contiguous(), float(pos[4].bias.detach()))
    self._key = key

  def _tconv_ok(self, m):
    return self.x3_conv and m.stride == (2, 2) and m.out_channels % 4 == 0      # 4 cout: a multiple of srl_tconv's 16

  def _family(self, m):
    """The hand-written kernel family of a convolution module, by its type and channel counts (None: the library convolution +
    the fused epilogues).  Whether the family's kernel takes the layer at a given map size and batch is the routers' business."""
    if not (self.mfma_conv or self.x3_conv):
      return None
    cin, cout = m.in_channels, m.out_channels
    if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3):
      if cin in (1, 2) and cout == 16:
        return 'thin'                # the first layers, on the vector ALU
      if cin in (16, 32, 64) and cout in (16, 32):
        return 'conv_mfma'           # csrc/conv_mfma.hip: bf16, or bf16x3 products in the fp32-class mode
      if cout in (64, 128, 256) and cin % 32 == 0:
        return 'gemm'                # the deep levels: implicit GEMM on the matrix cores (csrc/conv_gemm.hip)
    if isinstance(m, torch.nn.ConvTranspose2d) and m.kernel_size == (2, 2):
      if (cin, cout) in ((32, 16), (64, 32)):
        return 'convt_mfma'
      if (cin, cout) in ((128, 64), (256, 128)):
        return 'convt_gemm'
      # float32 rollout: any other 2 x 2 stride-2 transposed convolution as a 1 x 1 convolution to 4 cout channels +
      # depth-to-space in true float32 on the matrix cores (csrc/train_conv.hip k_tconv, the update's kernel)
      if self._tconv_ok(m):
        return 'tconv'
    return None

  def _mine(self, m, x):
    return m in self._wf and x.shape[2] % 16 == 0 and x.shape[3] % 16 == 0

  def _gemm(self, m, x):
    return m in self._wg and x.shape[2] == x.shape[3] and \
      conv3x3_gemm_supported(m.in_channels, m.out_channels, x.shape[3], x.shape[0])

  def _conv(self, m, x):
    w, b = self._w[m]
    return _cl(torch.nn.functional.conv2d(x, w, None, padding=m.padding)), b

  def _conv3x3(self, m, x, form='plain', cat=None, mfma=True, gemm=True):
    """relu(conv3x3(x) + bias) of module m by the first of conv_mfma, the implicit GEMM and the library convolution + epilogue
    that takes the layer at this map size and batch; mfma / gemm = False: that family is not tried at this position.
    form 'plain': returns the output, channels-last; 'nchw': NCHW-contiguous (the GEMM has no such store: gemm=False goes with it);
    'slice+pool': the output goes to the second half of the decoder's concat buffer `cat`, its 2 x 2 max-pool is returned."""
    f, b = m.out_channels, self._w[m][1]
    if mfma and self._mine(m, x):
      if form == 'slice+pool':
        return conv3x3_bias_relu(x, self._wf[m], b, f, out=cat, out_offset=f, pool=True)[1]
      return conv3x3_bias_relu(x, self._wf[m], b, f, nchw=form == 'nchw')
    if gemm and self._gemm(m, x):
      if form == 'slice+pool':
        conv3x3_gemm_bias_relu(x, self._wg[m], b, f, out=cat, out_offset=f)
        return pool2x2(cat, f, f)
      return conv3x3_gemm_bias_relu(x, self._wg[m], b, f)
    y, b = self._conv(m, x)
    return bias_act_pool(y, b, cat, f) if form == 'slice+pool' else bias_act(y, b, nchw=form == 'nchw')

  def _upconv(self, up, x, cat):
    """relu(conv_transpose2d(x, k=2, s=2) + bias) of module `up` into the first half of the concat buffer `cat`
    (Concatenate([up, skip]) without a copy)."""
    f, b = up.out_channels, self._w[up][1]
    cl = x.is_contiguous(memory_format=_CL)
    if up in self._wf and x.shape[3] % 16 == 0 and cl:
      convt2x2_bias_relu(x, self._wf[up], b, f, cat, 0)
    elif up in self._wg and cl:
      convt2x2_gemm_bias_relu(x, self._wg[up], b, f, cat, 0)
    elif up in self._w1 and x.dtype == torch.float32 and cl and cat.is_contiguous(memory_format=_CL):
      from stackrl_amd import qtrain                    # channels-last tensors are [B, H, W, C] in memory
      qtrain.tconv(qtrain.Act(x.permute(0, 2, 3, 1)), self._w1[up], b, 4 * f, taps=1, relu=True, out=(cat.permute(0, 2, 3, 1), 0), d2s=f)
    else:
      y = _cl(torch.nn.functional.conv_transpose2d(x, self._w[up][0], None, stride=up.stride))
      bias_act(y, b, out=cat, out_offset=0)

  def _unet(self, U, obs, bottom=False):
    """obs: the env's uint8 observation [B,H,W,c] (channels-last memory).  bottom: also return the bottleneck (the output of
    the bottom block), channels-last."""
    B = obs.shape[0]
    cats = []
    x = None
    for blk in U.down:
      f = blk[0].out_channels
      if x is None and self.fuse_thin and self.x3_conv and blk[0] in self._wt and blk[2] in self._wf and f == 16 and \
         blk[2].in_channels == 16 and obs.shape[1] % 16 == 0 and obs.shape[2] % 16 == 0:
        cat = torch.empty((B, 2 * f, obs.shape[1], obs.shape[2]), dtype=self.dtype, device=obs.device, memory_format=_CL)
        _, x = thin_conv3x3_bias_relu(obs, self._wt[blk[0]], self._w[blk[0]][1], self._wf[blk[2]], self._w[blk[2]][1],
                                      out=cat, out_offset=f, pool=True)
        cats.append(cat)
        continue
      if x is None and blk[0] in self._wt:
        y = conv3x3_thin(obs, self._wt[blk[0]], self._w[blk[0]][1], dtype=self.dtype)   # /255 and the cast happen in the kernel
      elif x is None:
        # uint8 NHWC / 255 (models.py:144-147); the NHWC memory is exactly a channels-last NCHW tensor
        x = (obs.float() / 255.0).to(self.dtype).permute(0, 3, 1, 2)
        y = self._conv3x3(blk[0], x, mfma=False, gemm=False)      # a first layer that is not thin stays with the library
      else:
        y = self._conv3x3(blk[0], x)
      cat = torch.empty((B, 2 * f, y.shape[2], y.shape[3]), dtype=y.dtype, device=y.device, memory_format=_CL)
      x = self._conv3x3(blk[2], y, 'slice+pool', cat)
      cats.append(cat)
    for m in (U.bottom[0], U.bottom[2]):
      x = self._conv3x3(m, x, mfma=False)                         # the bottom block tries only the GEMM
    x0 = x
    n = len(U.up)
    for k, (up, blk) in enumerate(zip(U.up, U.upconv)):
      cat = cats.pop()
      self._upconv(up, x, cat)
      y = self._conv3x3(blk[0], cat)
      last = k == n - 1                                           # the features leave NCHW-contiguous: never the GEMM
      x = self._conv3x3(blk[2], y, 'nchw' if last else 'plain', gemm=not last)
    return (x, x0) if bottom else x

  @torch.no_grad()
  def __call__(self, inputs):
    return self.features(inputs)

  @torch.no_grad()
  def features(self, inputs, bottom=False):
    """The left and right feature maps; bottom=True: (x, w, x0) with the left bottleneck x0 (what the value branch of the
    dueling head pools, models.py:179-186) as [B, h, w, C] in this object's dtype, contiguous."""
    self._refresh()
    xm, xo = inputs
    if not bottom:
      return self._unet(self.net.left, xm.contiguous()), self._unet(self.net.right, xo.contiguous())
    x, x0 = self._unet(self.net.left, xm.contiguous(), bottom=True)
    return x, self._unet(self.net.right, xo.contiguous()), x0.permute(0, 2, 3, 1).contiguous()

  @torch.no_grad()
  def pos(self, corr):
    """`pos_layers` (layers.py:439-472) on the correlation map [B,1,oh,ow] float32 -> advantages [B, oh*ow] float32:
    the 1 -> 16 layer on the vector ALU into a zero-margined map (of this object's dtype) padded to a multiple of 16, then
    the 16 -> 16 layer on the matrix cores with the final 1 x 1 projection fused into its epilogue (fp32 from the
    accumulators)."""
    self._refresh()
    if self._pos is None:
      return self.net.pos(corr).flatten(1)
    pos = self.net.pos
    B, _, oh, ow = corr.shape
    pw, pb = self._pos
    if self.fuse_thin and self.x3_conv:       # fp32-class: the three layers as one kernel, the 16-channel maps never leave LDS
      return thin_conv3x3_relu_project(corr.reshape(B, oh, ow).contiguous(), self._wt[pos[0]], self._w[pos[0]][1], self._wf[pos[2]],
                                       self._w[pos[2]][1], pw, pb).flatten(1)
    hp, wp = (oh + 15) // 16 * 16, (ow + 15) // 16 * 16
    key = (B, hp, wp, corr.device.index)
    buf = self._posbuf.get(key)
    if buf is None:
      buf = torch.zeros((B, 16, hp, wp), dtype=self.dtype, device=corr.device).contiguous(memory_format=_CL)
      self._posbuf = {key: buf}
    conv3x3_thin(corr.reshape(B, oh, ow, 1).contiguous(), self._wt[pos[0]], self._w[pos[0]][1], out=buf)
    return conv3x3_relu_project(buf, self._wf[pos[2]], self._w[pos[2]][1], pw, pb, oh, ow).flatten(1)


class FusedPolicy(object):
  """Rollout policy (`DQN.collect` -> `policy(exploration=True)`, dqn.py:391-395) with the hand-written head:
  library convs for the two U-Nets and the position convs, HIP cross-correlation, HIP arg-max + epsilon-greedy.
  Draws the same random numbers in the same order as `DQN.policy`, so both paths give identical actions.
  With mode='boltzmann' the head is `boltzmann_head`: the third argument of a call is the temperature and the draws are
  one Philox stream key per sample (include/stackrl_explore.h)."""

  def __init__(self, chunk=2048, autocast=None, fast=None):
    # rollout batches are processed in chunks to bound activation memory: 2,048 samples hold ~10 GB of fp32 activations
    # (of 288 GB) and run 4 % faster per sample than 512 (more workgroups per launch: 24.9 against 26.1 ms per 4,096, bf16)
    self.chunk = int(chunk)
    self.autocast = autocast     # None = fp32 like the reference; torch.bfloat16 runs the library convs on MFMA
    # fused epilogues around bias-free library convolutions (bf16: + the MFMA convolution kernels; fp32: epilogues only)
    self.fast = (autocast == torch.bfloat16) if fast is None else bool(fast)
    self._ff = None

  def _fast(self, net):
    """The `FastFeatures` of `net` (one object, rebuilt when another net arrives)."""
    if self._ff is None or self._ff.net is not net:
      self._ff = FastFeatures(net, dtype=torch.bfloat16 if self.autocast == torch.bfloat16 else torch.float32)
    return self._ff

  ROUTING_BATCH = 8   # the largest batch multiple a layer's routing looks at (srl_conv3x3_gemm_batch_multiple)

  @staticmethod
  def draws(net, B, gen, device, mode='epsilon-greedy'):
    """The random numbers one call over B samples consumes, drawn as that call draws them (`draws=` of `__call__`: a
    policy evaluated group by group passes each group its slice and takes the actions of one call over the batch)."""
    if mode == 'boltzmann':
      return (torch.randint(0, 2 ** 32, (B, 2), dtype=torch.int64, generator=gen, device=device),)
    u = torch.rand(B, generator=gen, device=device)
    return u, torch.randint(net.n_actions, (B,), generator=gen, device=device)

  @torch.no_grad()
  def __call__(self, net, inputs, epsilon, gen, draws=None, mode='epsilon-greedy'):
    if mode not in ('epsilon-greedy', 'boltzmann'):
      raise ValueError("Invalid value {} for argument mode. Must be 'epsilon-greedy' or 'boltzmann'.".format(mode))
    xm, xo = inputs
    B = xm.shape[0]
    if draws is None:
      draws = self.draws(net, B, gen, xm.device, mode)
    if mode == 'boltzmann':
      keys, = draws
    else:
      u, rnd = draws
    out = torch.empty(B, dtype=torch.int64, device=xm.device)
    for s in range(0, B, self.chunk):
      e = min(B, s + self.chunk)
      if self.fast:
        x, w = self._fast(net)((xm[s:e], xo[s:e]))
      elif self.autocast is not None:
        with torch.autocast('cuda', dtype=self.autocast):
          x, _, w = net.features((xm[s:e], xo[s:e]))
      else:
        x, _, w = net.features((xm[s:e], xo[s:e]))
      corr = xcorr_forward(x, w)
      adv = self._ff.pos(corr) if self.fast else net.pos(corr).flatten(1)
      out[s:e] = boltzmann_head(adv, keys[s:e], epsilon) if mode == 'boltzmann' else policy_head(adv, u[s:e], rnd[s:e], epsilon)
    return out


  # ---------------------------------------------------------------------------------------------- greedy acting, evaluation
  def _features(self, net, xm, xo):
    """(left features, right features, left bottleneck [B, h, w, C]) of one chunk, by the path `__call__` takes."""
    if self.fast:
      return self._fast(net).features((xm, xo), bottom=True)
    prep = net.prepare((xm, xo))
    if self.autocast is not None:
      with torch.autocast('cuda', dtype=self.autocast):
        (x, x0), (w, _) = net.left(prep[0]), net.right(prep[1])
    else:
      (x, x0), (w, _) = net.left(prep[0]), net.right(prep[1])
    return x, w, x0.permute(0, 2, 3, 1).contiguous()

  @torch.no_grad()
  def state_value(self, net, x0):
    """The state value of the dueling head (`layers.value`, layers.py:424-436; models.py:179-186) from the left bottleneck
    x0 [B, h, w, C]: float32 [B], or None for a net without the dueling head.  Average pooling: `srl_tvalue_fwd`, the kernel
    of the update, on the float32 view of x0 with the weights of `net.value`; any other head: the module's own layers."""
    if not getattr(net, 'dueling', False):
      return None
    B, h, w, C = x0.shape
    x0 = x0.float().contiguous()
    val = net.value
    if net.dueling_avg_pool and len(val) == 3 and isinstance(val[0], torch.nn.Linear) and isinstance(val[2], torch.nn.Linear) and \
       val[2].out_features == 1 and C <= 4096:
      d1, d2 = val[0], val[2]
      W1, b1, W2, b2 = (t.detach().float().contiguous() for t in (d1.weight, d1.bias, d2.weight, d2.bias))
      v = torch.empty(B, dtype=torch.float32, device=x0.device)
      call('srl_tvalue_fwd', x0, x0, W1, b1, W2, b2, None, None, v, B, h * w, C, int(d1.out_features))
      return v
    pooled = x0.mean(dim=(1, 2)) if net.dueling_avg_pool else x0.amax(dim=(1, 2))
    return val(pooled).reshape(B)

  @torch.no_grad()
  def greedy(self, net, inputs, n_valid=None, stats=False, values=False):
    """Greedy acting on the rollout kernels (the head: include/stackrl_greedy.h): the forward of `__call__`, the state value,
    then `greedy_head` — no [B, A] Q tensor unless `values` asks for it.  inputs[1] is [B, h, w, 1], or the Stack-v2 layout
    of the vectorised env [B, G, h, w, 1] (G object maps per overhead map, the first `n_valid` valid): the left U-Net and the
    value run once per env, the right U-Net on the B * G maps, and the action is r * A + p.  `chunk` counts
    cross-correlation samples: an env chunk is chunk // G, rounded down to a multiple of ROUTING_BATCH (and at least that).
    Returns actions [B] i64, then as asked stats [B, 4] f64 {max, min, sum, sum of squares of Q} and Q [B, G * A] f32."""
    xm, xo = inputs
    B = xm.shape[0]
    grouped = xo.dim() == 5
    G = xo.shape[1] if grouped else 1
    if n_valid is not None and not 1 <= int(n_valid) <= G:
      raise ValueError('n_valid must be in 1..{}, got {}'.format(G, n_valid))
    # every chunk is evaluated as a multiple of ROUTING_BATCH envs (the last one padded with blank observations): which kernel
    # a deep layer goes to depends on the batch (FastFeatures._gemm), and the cross-correlation is the row-product kernel at every
    # batch size (`xcorr_forward_rows`); the hand-written kernels work sample by sample, so where no layer falls to the library
    # (128 / 32, fp32-class) an env's result does not depend on the chunk size or on the batch it arrives in
    R = self.ROUTING_BATCH
    step = max(R, self.chunk // G // R * R)
    actions = torch.empty(B, dtype=torch.int64, device=xm.device)
    st = torch.empty((B, 4), dtype=torch.float64, device=xm.device) if stats else None
    q = None
    for s in range(0, B, step):
      e = min(B, s + step)
      cm, co = xm[s:e], xo[s:e]
      n = e - s + (s - e) % R
      if n > e - s:
        cm = torch.cat((cm, cm.new_zeros((n - (e - s),) + tuple(cm.shape[1:]))))
        co = torch.cat((co, co.new_zeros((n - (e - s),) + tuple(co.shape[1:]))))
      x, w, x0 = self._features(net, cm, co.reshape(n * G, *co.shape[-3:]) if grouped else co)
      v = self.state_value(net, x0)
      if G > 1:                                    # the env's left feature map once per object map
        x = x[:, None].expand(n, G, *x.shape[1:]).reshape(n * G, *x.shape[1:])
      corr = xcorr_forward_rows(x, w)
      adv = (self._ff.pos(corr) if self.fast else net.pos(corr).flatten(1)).reshape(n, G, -1)[:e - s]
      v = v[:e - s] if v is not None else None
      out = greedy_head(adv, v, n_valid, stats=stats, values=values)
      out = out if isinstance(out, tuple) else (out,)
      actions[s:e] = out[0]
      if stats:
        st[s:e] = out[1]
      if values:
        qc = out[-1].reshape(e - s, -1)
        if q is None:
          q = qc if e - s == B else torch.empty((B, qc.shape[1]), dtype=torch.float32, device=xm.device)
        if q is not qc:
          q[s:e] = qc
    out = (actions,) + ((st,) if stats else ()) + ((q,) if values else ())
    return out if len(out) > 1 else actions


# ------------------------------------------------------------------------------------------------ update path (csrc/learner.hip)
def td_epilogue(q, q_next_online, q_next_target, actions, rewards, terminal, weights, gamma, huber_delta, reward_scale,
                double, prio_eps, ws):
  """Loss, mean TD, |TD|, new priorities and d loss / d Q(s, .) of `DQN.train` (dqn.py:408-476) in one launch.
  q, q_next_*: float32 [mb, A]; ws: a dict the caller keeps (scratch and the ticket word live at fixed addresses)."""
  mb, A = q.shape
  dev = q.device
  if 'ticket' not in ws or ws['mb'] != mb:
    ws.update(mb=mb, ticket=torch.zeros(1, dtype=torch.int32, device=dev), scratch=torch.empty(2 * mb, dtype=torch.float32, device=dev))
  out = torch.empty(2, dtype=torch.float32, device=dev)
  td_abs = torch.empty(mb, dtype=torch.float32, device=dev)
  logits = torch.empty(mb, dtype=torch.float32, device=dev)
  grad_q = torch.empty((mb, A), dtype=torch.float32, device=dev)
  q = q.contiguous(); qt = q_next_target.contiguous()
  qo = q_next_online.contiguous() if q_next_online is not None else None
  term = terminal.contiguous().view(torch.uint8)
  act = actions.contiguous(); rew = rewards.contiguous().float()
  wts = weights.contiguous().float() if weights is not None else None
  call('srl_td_epilogue', q, q, qo, qt, act, rew, term, wts, float(gamma), -1.0 if huber_delta is None else float(huber_delta),
       float(reward_scale or 0.0), int(bool(double)), float(prio_eps), mb, A, out, out[1:], td_abs, logits, grad_q, ws['scratch'], ws['ticket'])
  return out[0], out[1], td_abs, logits, grad_q


def adam_step(params, grads, m, v, state, lr, beta1, beta2, eps):
  """Keras Adam over flat fp32 buckets, in place; `state` = 4 device floats {t, beta1^t, beta2^t, lr_t}."""
  call('srl_adam_step', params, params, grads, m, v, params.numel(), state, float(lr), float(beta1), float(beta2), float(eps))


def gumbel_topk(logits, u, alpha_t, k, ws):
  """K7: indices (int64 [k], descending key) and keys of the k largest alpha * logit + Gumbel(u)."""
  n = logits.numel()
  need = load().srl_gumbel_topk_scratch_bytes(n, k)
  if ws.get('topk_n') != (n, k):
    ws['topk_n'] = (n, k)
    ws['topk_scratch'] = torch.empty(need, dtype=torch.uint8, device=logits.device)
  idx = torch.empty(k, dtype=torch.int64, device=logits.device)
  key = torch.empty(k, dtype=torch.float32, device=logits.device)
  call('srl_gumbel_topk', logits, logits, u, alpha_t, n, k, idx, key, ws['topk_scratch'], need)
  return idx, key


def replay_scatter(state, reward, terminal, action, slot, part_len, mem_states, mem_reward, mem_terminal, mem_action, mem_logits):
  """K8: one transition per env into row b * part_len + slot of the replay tensors (memory.py:153-161)."""
  s0, s1 = (t.contiguous() for t in state)
  B = s0.shape[0]
  b0, b1 = s0[0].numel() * s0.element_size(), s1[0].numel() * s1.element_size()
  r = reward.contiguous().float(); t = terminal.contiguous().to(torch.bool).view(torch.uint8); a = action.contiguous().to(torch.int64)
  call('srl_replay_scatter', s0, s0, s1, b0, b1, r, t, a, B, int(slot), int(part_len), mem_states[0], mem_states[1], mem_reward,
       mem_terminal, mem_action, mem_logits)


def logit_extrema(logits, ws):
  """(max logit, its lowest index), (min finite logit, its lowest index) as four 0-dim tensors (`ReplayMemory`'s tracker
  scans, memory.py:164-177, :282-316).  ws: a dict the caller keeps (scratch at a fixed address: hipGraph replay)."""
  dev = logits.device
  if 'ext' not in ws:
    ws['ext'] = torch.empty(int(load().srl_logit_extrema_scratch_bytes()), dtype=torch.uint8, device=dev)
  v = torch.empty(2, dtype=torch.float32, device=dev)
  i = torch.empty(2, dtype=torch.int64, device=dev)
  call('srl_logit_extrema', logits, logits, logits.numel(), v, i, ws['ext'])
  return (v[0], i[0]), (v[1], i[1])


def replay_gather(idx, part_len, n_steps, literal_next, mem_states, mem_reward, mem_terminal, mem_action, mem_logits,
                  alpha_t=None, beta_t=None, min_logit=None):
  """K8: the minibatch for the sampled rows (memory.py:232-260): (states, actions, rewards, next_states, terminal), weights."""
  mb = idx.numel()
  m0, m1 = mem_states
  dev = m0.device
  b0, b1 = m0[0].numel() * m0.element_size(), m1[0].numel() * m1.element_size()
  s0 = torch.empty((mb,) + tuple(m0.shape[1:]), dtype=m0.dtype, device=dev); n0 = torch.empty_like(s0)
  s1 = torch.empty((mb,) + tuple(m1.shape[1:]), dtype=m1.dtype, device=dev); n1 = torch.empty_like(s1)
  act = torch.empty(mb, dtype=torch.int64, device=dev)
  rew = torch.empty(mb, dtype=torch.float32, device=dev)
  term = torch.empty(mb, dtype=torch.bool, device=dev)
  w = torch.empty(mb, dtype=torch.float32, device=dev) if alpha_t is not None else None
  call('srl_replay_gather', m0, idx, mb, int(part_len), int(n_steps), int(bool(literal_next)), None, m0, m1, b0, b1, mem_reward,
       mem_terminal, mem_action, mem_logits, alpha_t, beta_t, min_logit, s0, s1, n0, n1, act, rew, term, w)
  return ((s0, s1), act, rew, (n0, n1), term), w
