"""The candidates of a lookahead, spread over the value map by greedy non-maximum suppression: candidate 0 is the base policy's
action, and every further candidate is the best entry that lies more than `radius` pixels (Chebyshev, within its own map) from
all the candidates before it.  include/stackrl_candidates.h states the definition, csrc/candidates.hip holds the kernel
(libstackrl_candidates.so), tests/candidates_cases.py the numpy restatement.

`select` serves device tensors with the kernel and CPU tensors with `select_reference`, the same definition as a torch
composition (k rounds of arg-max and masking).  At radius 0 both give `lookahead.candidates`."""
import ctypes

import torch

from stackrl_amd import _bind

MAX_K = 32

_VP, _I32, _INT = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int
# export -> (restype, argtypes, error accessor or None): every declaration of include/stackrl_candidates.h (pointers as void*);
# tests/test_abi.py holds the table to the header and the library.
_SIGS = {
  'srl_candidates_select': (_INT, [_VP, _I32, _VP] + [_I32] * 6 + [_VP] * 3, 'srl_candidates_last_error'),
  'srl_candidates_last_error': (ctypes.c_char_p, [], None),
  'srl_candidates_build_info': (ctypes.c_char_p, [], None),
}

load, call = _bind.binding('candidates', _SIGS)


def _arguments(values, action, k, radius, n_valid, OH):
  """(values [B, G, A] float32 or float64 contiguous, action int64 [B] or None, B, G, OH, n_valid, k, radius), checked."""
  values = torch.as_tensor(values)
  if values.dim() < 2:
    raise ValueError('values must be [B, A] or [B, G, A], got {}'.format(tuple(values.shape)))
  if values.dtype not in (torch.float32, torch.float64):
    values = values.float()
  B = int(values.shape[0])
  values = values.reshape(B, -1).contiguous()
  N = int(values.shape[1])
  if B < 1 or N < 1:
    raise ValueError('values must hold at least one env and one entry, got {}'.format(tuple(values.shape)))
  if OH is None:
    if n_valid is not None:
      raise ValueError('n_valid needs OH: the maps of an env cannot be told apart without it')
    OH = int(round(N ** 0.5))               # one square map
  OH = int(OH)
  A = OH * OH
  if OH < 1 or N % A:
    raise ValueError('the {} entries of an env are no whole number of {} x {} maps'.format(N, OH, OH))
  G = N // A
  n_valid = G if n_valid is None else int(n_valid)
  k, radius = int(k), int(radius)
  if not 1 <= n_valid <= G:
    raise ValueError('n_valid must be in 1..{}, got {}'.format(G, n_valid))
  if not 1 <= k <= MAX_K:
    raise ValueError('k must be in 1..{}, got {}'.format(MAX_K, k))
  if radius < 0:
    raise ValueError('radius must be at least 0, got {}'.format(radius))
  if G * A > 2 ** 31 - 2:
    raise ValueError('G * A must be at most 2^31-2, got {} * {}'.format(G, A))
  if action is not None:
    action = torch.as_tensor(action).to(device=values.device, dtype=torch.int64).reshape(-1).contiguous()
    if action.shape[0] != B:
      raise ValueError('action must be [{}], got {}'.format(B, tuple(action.shape)))
  return values.reshape(B, G, A), action, B, G, OH, n_valid, k, radius


def select(values, action=None, k=8, radius=0, n_valid=None, OH=None):
  """(cand int64 [B, k], count int32 [B]) of include/stackrl_candidates.h on the device of `values` [B, G * A] (or
  [B, G, A]): float32 and float64 tensors go to the kernel as they are, other dtypes and non-contiguous tensors as contiguous
  float32.  `OH`: the side of a map (default: the entries of an env are one square map).  One launch on the current stream of
  a device tensor; a CPU tensor is served by `select_reference`."""
  values, action, B, G, OH, n_valid, k, radius = _arguments(values, action, k, radius, n_valid, OH)
  if not values.is_cuda:
    return _reference(values, action, B, G, OH, n_valid, k, radius)
  cand = torch.empty((B, k), dtype=torch.int64, device=values.device)
  count = torch.empty((B,), dtype=torch.int32, device=values.device)
  call('srl_candidates_select', values, values, int(values.dtype == torch.float64), action, B, G, OH, n_valid, k, radius, cand, count)
  return cand, count


def select_reference(values, action=None, k=8, radius=0, n_valid=None, OH=None):
  """`select` as a torch composition on the device of `values`: k rounds of arg-max and masking."""
  return _reference(*_arguments(values, action, k, radius, n_valid, OH))


def _reference(values, action, B, G, OH, n_valid, k, radius):
  dev = values.device
  A = OH * OH
  N = n_valid * A
  # the order of the definition as one int64 key per entry (float32 -> float64 is exact and keeps every tie and no other):
  # NaN above everything, -0 with +0, then the bits of the double made monotone
  v = values.reshape(B, G * A)[:, :N].double()
  bits = (v + 0.0).view(torch.int64)
  key = bits ^ ((bits >> 63) & 0x7fffffffffffffff)
  key = torch.where(torch.isnan(v), torch.full_like(key, 2 ** 63 - 1), key)
  struck_key = -2 ** 63                                     # below the key of -inf
  index = torch.arange(N, device=dev)
  g, y, x = index // A, (index % A) // OH, index % OH
  struck = torch.zeros((B, N), dtype=torch.bool, device=dev)

  def strike(i):
    gi, yi, xi = (i // A)[:, None], ((i % A) // OH)[:, None], (i % OH)[:, None]
    return (g[None] == gi) & ((y[None] - yi).abs() <= radius) & ((x[None] - xi).abs() <= radius)

  cand = torch.empty((B, k), dtype=torch.int64, device=dev)
  count = torch.ones((B,), dtype=torch.int32, device=dev)
  alive = torch.ones((B,), dtype=torch.bool, device=dev)
  for c in range(k):
    if c == 0 and action is not None:
      pick = action.clamp(0, G * A - 1)
    else:
      masked = torch.where(struck, torch.full_like(key, struck_key), key)
      best = masked.max(dim=1).values
      pick = torch.where(masked == best[:, None], index[None], torch.full_like(index, N)[None]).min(dim=1).values
      alive = alive & ~struck.all(dim=1)
      if c:
        count += alive.to(torch.int32)
      pick = torch.where(alive, pick, cand[:, 0])
    cand[:, c] = pick
    struck = struck | (strike(pick) & alive[:, None])
  return cand, count
