"""Operands for which the matrix-core cross-correlation (csrc/xcorr_mfma.hip) has ONE right answer in float32, and that answer
in float64 (no GPU).  Shared by tests/test_xcorr_cases.py (the builders, on the CPU) and tests/test_xcorr_exact_gpu.py (the
kernels, bit for bit).

The kernels multiply bf16 values on the matrix cores and add in float32, in an order that differs from kernel to kernel
(Toeplitz fragments per kernel row, Hankel fragments per map row, partial sums per channel group, per wave, per half row).  If
every product and every partial sum OF ANY ORDER is a float32 value, no order can round, and every kernel has to return the
float64 result exactly.  The condition: every term is a multiple of one unit (`lsb`), and the sum of the terms' magnitudes is at
most 2^22 units at every output — a factor 4 under the 2^24 consecutive multiples float32 holds.  Each builder computes that sum
(`bound`, in units, the largest over the case's outputs) and asserts it.

  * integer operands (`int_case`): maps in {0 .. 3}, kernels and output gradients in {-2 .. 2}, drawn independently per sample,
    channel and position.  Exact in bf16, so they serve every operand dtype at precision 0, and the lo planes of the split are
    zero.  lsb = 1; |sum| <= 16,384 x 6 = 2^16.6 forward, 9,409 x 6 = 2^15.8 for d/dw.
  * split operands (`split_case`), for precision 1 (bf16x3): v = h + l with h a small integer and l = +-2^-10 (or 0; 0 where
    h = 0), so that bf16(v) = h and bf16(v - h) = l exactly, without ties — `split_bf16` is the host's restatement of
    `srl_split_bf16` and returns exactly these planes.  The expectation is the header's sum, hi hi' + hi lo' + lo hi' (the
    lo lo' term is dropped), lsb = 2^-10.  Maps are dense (h in {0, 1, 2}; the gradient map of d/dx +-{1, 2}); the OTHER
    operand is sparse to keep the sum of magnitudes under the bound: kernels carry `taps_per_kernel` taps of h = +-1, dealt from
    shuffled runs of all tap positions, so that the (sample, channel) kernels of a case use every tap position; the output
    gradient of d/dw carries every third position, offset by the sample.  Sparse operands always carry a lo part.

The three modes as the kernel sees them (`op`): a map correlated with a per-sample kernel,
    0  forward  a = x  [B, C, H, H],            k = w        [B, C, h, h]  ->  [B, 1, O, O]   (channels summed)
    1  d/dx     a = gp [B, O + 2 (h - 1), ..],  k = w flipped [B, C, h, h]  ->  [B, C, H, H]
    2  d/dw     a = x  [B, C, H, H],            k = g        [B, O, O]     ->  [B, C, h, h]
`corr64` evaluates them in float64 as one matrix product per map (rows of windows times the kernel's rows, summed along the
diagonal); every sum in it is exact, so it equals `nets.correlation_reference` and its autograd gradients bit for bit — which
tests/test_xcorr_cases.py asserts at both geometries — at a hundredth of their CPU time (47 s for the gradients of 32 samples)."""
import functools

import numpy as np
import torch

GEOMETRIES = ((128, 32), (64, 16))
LIMIT = 2.0 ** 22             # units: the condition every case meets
LO = 2.0 ** -10               # the lo parts' magnitude = the unit of a split case


# ------------------------------------------------------------------------------------------------ the host's bf16 split
def split_bf16(v):
  """`srl_split_bf16` on the host: hi = bf16(v), lo = bf16(v - hi), both round-to-nearest-even, returned as float32."""
  v = v.float()
  hi = v.to(torch.bfloat16).float()
  return hi, (v - hi).to(torch.bfloat16).float()


def truncate_bf16(v):
  """The WRONG conversion: the upper 16 bits of the float32 (round towards zero)."""
  return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


# ------------------------------------------------------------------------------------------------ float64 evaluation
def corr64(m, k, chunk=64):
  """out[n, y, x] = sum_{i, t} m[n, y + i, x + t] k[n, i, t] in float64: m [N, Hm, Hm], k [N, K, K]."""
  m, k = m.double(), k.double()
  N, Hm, K = m.shape[0], m.shape[-1], k.shape[-1]
  O = Hm - K + 1
  out = torch.empty((N, O, O), dtype=torch.float64)
  for a in range(0, N, chunk):
    mu = m[a:a + chunk].unfold(-1, K, 1)                                                    # [n, Hm, O, K]: windows of every row
    n = mu.shape[0]
    z = torch.bmm(mu.reshape(n, Hm * O, K), k[a:a + chunk].transpose(-1, -2)).reshape(n, Hm, O, K)   # row rho x kernel row i
    s = z.stride()
    out[a:a + chunk] = z.as_strided((n, O, O, K), (s[0], s[1], s[2], s[1] + s[3])).sum(-1)   # sum_i z[y + i, x, i]
  return out


def op(mode, a, k, corr=corr64):
  """One mode of srl_xcorr_mfma on its own operands (module docstring), float64: B C correlations of one map with one kernel
  (`corr`), the forward's summed over the channels."""
  B, C = k.shape[:2] if mode == 1 else a.shape[:2]
  m = a.repeat_interleave(C, 0) if mode == 1 else a.reshape((B * C,) + a.shape[-2:])
  kk = k.repeat_interleave(C, 0) if mode == 2 else k.reshape((B * C,) + k.shape[-2:])
  r = corr(m, kk)
  r = r.reshape((B, C) + r.shape[-2:])
  return r.sum(1, keepdim=True) if mode == 0 else r


def expectation(mode, a, k, split, magnitudes=True):
  """(what the kernel must return, the sum of its terms' magnitudes or None), float64.  Precision 0 (`split` false): the
  operands rounded to bf16, multiplied and summed.  Precision 1: hi hi' + hi lo' + lo hi' of the split operands — by
  bilinearity (hi + lo)(hi' + lo') - lo lo', every sum exact in float64 for this module's operands."""
  ah, al = (t.double() for t in split_bf16(a))
  kh, kl = (t.double() for t in split_bf16(k))
  if not split:
    return op(mode, ah, kh), op(mode, ah.abs(), kh.abs()) if magnitudes else None
  return (op(mode, ah + al, kh + kl) - op(mode, al, kl),
          op(mode, ah.abs() + al.abs(), kh.abs() + kl.abs()) - op(mode, al.abs(), kl.abs()) if magnitudes else None)


def pad_gradient(g, h):
  """`srl_tcorr_grad`'s second output: the output gradient [B, O, O] between h - 1 zeros on every side."""
  return torch.nn.functional.pad(g, (h - 1,) * 4)


def flip(w):
  """`srl_tflip`: the kernels turned by 180 degrees."""
  return w.flip(-1, -2)


def operands(case, mode):
  """(a, k) of `op` for a case: float32 host tensors."""
  if mode == 0:
    return case['x'], case['w']
  if mode == 1:
    return pad_gradient(case['g_dx'], case['h']), flip(case['w'])
  return case['x'], case['g_dw']


def _finish(case, split, lsb):
  case.update(split=split, lsb=lsb, expect={}, bound={})
  return case


def expect(case, mode):
  """The float64 result of `mode` for an exact case, as the float32 tensor a kernel must return bit for bit; computed at first
  use, kept, and shared (do not write to it).  case['bound'][mode] is the largest sum of magnitudes, in units."""
  if mode not in case['expect']:
    a, k = operands(case, mode)
    e, terms = expectation(mode, a, k, case['split'])
    lsb = case['lsb']
    case['bound'][mode] = float(terms.max()) / lsb
    assert case['bound'][mode] <= LIMIT, ('the sum of magnitudes must stay under 2^22 units', mode, case['bound'][mode])
    assert torch.equal(e.float().double(), e) and torch.equal((e / lsb).round() * lsb, e)     # a float32 value, in whole units
    case['expect'][mode] = e.float()
  return case['expect'][mode]


def _gen(kind, B, C, H, h):
  return torch.Generator().manual_seed(1000003 * kind + 7919 * B + 131 * C + H)


def _ints(gen, shape, lo, hi):
  return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _gaps(t, dims):
  """Where a position is zero in every sample (and channel): true at the FIRST sample (and channel) of those positions."""
  first = torch.zeros(t.shape[:dims] + (1,) * (t.dim() - dims), dtype=torch.bool)
  first.view(-1)[0] = True
  return ~(t != 0).any(tuple(range(dims)), keepdim=True) & first


@functools.lru_cache(maxsize=None)
def int_case(B, C, H, h):
  """Integer operands (module docstring).  Small cases leave positions that every sample's independent draw left zero (three
  draws of one channel are all zero at one position in 64): those take a 1 in the first sample, so that every map and tap
  position of every case carries a value.  The returned tensors are shared: do not write to them."""
  gen = _gen(1, B, C, H, h)
  O = H - h + 1
  x, w, g = _ints(gen, (B, C, H, H), 0, 3), _ints(gen, (B, C, h, h), -2, 2), _ints(gen, (B, O, O), -2, 2)
  for t, dims in ((x, 2), (w, 2), (g, 1)):
    t.masked_fill_(_gaps(t, dims), 1.0)
  return _finish(dict(B=B, C=C, H=H, h=h, x=x, w=w, g_dx=g, g_dw=g), False, 1.0)


def taps_per_kernel(B, C, h):
  """16, or as many as it takes for the B C kernels of a case to use every one of the h h tap positions."""
  return max(16, -(-h * h // (B * C)))


def _lo(gen, shape, zero=True):
  """Lo parts in units: -1, 0 or 1 (`zero`), or -1 or 1."""
  return (torch.randint(-1, 2, shape, generator=gen) if zero else 2 * torch.randint(0, 2, shape, generator=gen) - 1).float()


def _sign(gen, shape):
  return (2 * torch.randint(0, 2, shape, generator=gen) - 1).float()


@functools.lru_cache(maxsize=None)
def split_case(B, C, H, h):
  """Split operands (module docstring); `parts` holds the (h, l) planes each operand was built from."""
  gen = _gen(2, B, C, H, h)
  O = H - h + 1
  xh = _ints(gen, (B, C, H, H), 0, 2)
  xl = _lo(gen, xh.shape) * (xh != 0) * LO
  gap = _gaps(xl, 2)                       # positions without a lo part in any sample and channel (few channels): 1 + 2^-10
  xh, xl = torch.where(gap & (xh == 0), torch.ones_like(xh), xh), torch.where(gap, torch.full_like(xl, LO), xl)
  # kernels: taps from shuffled runs of all positions, `taps_per_kernel` to each (sample, channel) in turn (a position a kernel
  # is dealt twice, across the end of a run, counts once)
  n = taps_per_kernel(B, C, h)
  runs = -(-B * C * n // (h * h))
  deal = torch.cat([torch.randperm(h * h, generator=gen) for _ in range(runs)])[:B * C * n].reshape(B * C, n)
  mask = torch.zeros((B * C, h * h)).scatter_(1, deal, 1.0).reshape(B, C, h, h)
  wh = _sign(gen, mask.shape) * mask
  wl = _lo(gen, mask.shape, zero=False) * mask * LO
  # the gradient as the map of d/dx: dense, never zero; as the kernel of d/dw: every third position, offset by the sample
  gh = _sign(gen, (B, O, O)) * _ints(gen, (B, O, O), 1, 2)
  gl = _lo(gen, gh.shape, zero=False) * LO
  third = ((torch.arange(O * O).reshape(1, O, O) + torch.arange(B).reshape(B, 1, 1)) % 3 == 0).float()
  sh = _sign(gen, (B, O, O)) * third
  sl = _lo(gen, sh.shape, zero=False) * third * LO
  case = dict(B=B, C=C, H=H, h=h, x=xh + xl, w=wh + wl, g_dx=gh + gl, g_dw=sh + sl,
              parts=dict(x=(xh, xl), w=(wh, wl), g_dx=(gh, gl), g_dw=(sh, sl)))
  return _finish(case, True, LO)


# ------------------------------------------------------------------------------------------------ the one case with a tolerance
ROUNDING_TOL = 2e-5     # of the result's scale: the project's bound for exact bf16 operands (test_xcorr_mfma_bf16_matches_torch)


@functools.lru_cache(maxsize=None)
def rounding_case(B, C, H, h):
  """Dense random float32 operands as in tests/test_learner_gpu.py, for precision 0."""
  gen = _gen(3, B, C, H, h)
  O = H - h + 1
  g = torch.randn((B, O, O), generator=gen)
  return dict(B=B, C=C, H=H, h=h, x=torch.rand((B, C, H, H), generator=gen), w=torch.rand((B, C, h, h), generator=gen) - 0.3,
              g_dx=g, g_dw=g, refs={})


def rounding_refs(case, mode):
  """(the float64 correlation of the operands ROUNDED TO BF16, nearest even; that of the operands as they are)."""
  if mode not in case['refs']:
    a, k = operands(case, mode)
    case['refs'][mode] = (op(mode, a.to(torch.bfloat16), k.to(torch.bfloat16)), op(mode, a, k))
  return case['refs'][mode]


def ratio(got, want):
  """Max-norm error relative to the tensor's scale, as the existing cross-correlation tests state their tolerances."""
  return float((got.double() - want).abs().max()) / float(want.abs().max())


# ------------------------------------------------------------------------------------------------ plain loops, and wrong ones
def np_corr(m, k, shifted_tap=None):
  """`corr64` as a loop over the kernel's taps (numpy, float64).  `shifted_tap` = (n, i, t): THE DEFECT of reading that one
  tap's map values one column to the right."""
  m, k = np.asarray(m, np.float64), np.asarray(k, np.float64)
  K = k.shape[-1]
  O = m.shape[-1] - K + 1
  out = np.zeros((m.shape[0], O, O))
  for i in range(K):
    for t in range(K):
      for n in range(m.shape[0]):
        s = 1 if (n, i, t) == shifted_tap else 0
        out[n] += m[n, i:i + O, t + s:t + s + O] * k[n, i, t]
  return torch.from_numpy(out)


def corr64_shifted(m, k, shifted_tap):
  """The same defect on `corr64`: the one tap's contribution taken out and put back from one column to the right."""
  n, i, t = shifted_tap
  O = m.shape[-1] - k.shape[-1] + 1
  out = corr64(m, k)
  out[n] += (m[n, i:i + O, t + 1:t + 1 + O].double() - m[n, i:i + O, t:t + O].double()) * k[n, i, t].double()
  return out


DEFECTS = ('one tap shifted by a column', 'lo plane of the map\'s last column zeroed', 'one channel dropped', 'truncation')


def defective(mode, a, k, split, defect, loops=False):
  """What a kernel with ONE deliberate defect returns for the operands (a, k) of `mode`, float64; `loops`: by the plain numpy
  loop instead of `corr64`.  The shifted tap is the first non-zero tap, left of the last column, of the last map's kernel; the
  dropped channel is the last one's term of the forward's sum."""
  ah, al = split_bf16(a)
  kh, kl = split_bf16(k)
  corr = np_corr if loops else corr64
  if defect == DEFECTS[0]:
    n = (k.shape[0] * (a.shape[1] if mode == 2 else k.shape[1])) - 1
    last = kh[-1] if mode == 2 else kh[-1, -1]
    i, t = (last[:, :-1] != 0).nonzero()[0].tolist()
    corr = functools.partial(np_corr if loops else corr64_shifted, shifted_tap=(n, i, t))
  elif defect == DEFECTS[1]:
    assert split
    al = al.clone(); al[..., -1] = 0.0
  elif defect == DEFECTS[2]:
    assert mode == 0
    kh, kl = kh.clone(), kl.clone(); kh[:, -1] = 0.0; kl[:, -1] = 0.0
  elif defect == DEFECTS[3]:
    assert not split
    ah, kh = truncate_bf16(a), truncate_bf16(k)
  out = op(mode, ah, kh, corr)
  if split:
    out = out + op(mode, ah, kl, corr) + op(mode, al, kh, corr)
  return out
