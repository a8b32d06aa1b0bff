"""Heuristic baseline policies (`stackrl/baselines.py`) on the device: the reference's quality yardstick and its
optional initial-collect policy (`training.py:256-263`, `config.gin:118`, `:142`).

`Baseline(method=..., goal=True, minorder=1)` mirrors `stackrl.Baseline` (baselines.py:168-217): called with a batch of
observations it returns one flat action per env (and the negated value maps with `value=True`).  The sliding-window
value maps and the selection run in libstackrl_qnet.so (csrc/heuristics.hip); there is no CPU fallback.
`random` (baselines.py:145-150) draws uniform values with torch's generator (numpy's default_rng stream is not reproduced).

On Stack-v2 the vectorised env's observation holds G object maps per env over one overhead map ([B, G, h, w, 1]).  There the
policy is the reference's `Baseline(batched=True, batchwise=True)` (`__main__.py:111-117`): the selection per object map, then
the map whose returned value at its own action is the largest.  include/stackrl_baseline_rows.h states it; `Baseline`,
`heuristic_values` and `select` take that layout as it is, `baseline_rows_reference` restates the choice on the CPU.
"""
import numpy as np
import torch

from stackrl_amd import qops

METHODS = {'random': 0, 'correlate': 1, 'height': 2, 'difference': 3, 'corrcoef': 4}   # baselines.py:158-165
_lib = qops.load      # the library's one loader, under the name this module's callers used before `qops._SIGS` declared every export


def _check_n_valid(n_valid, G):
  n_valid = G if n_valid is None else int(n_valid)
  if not 1 <= n_valid <= G:
    raise ValueError('n_valid must be in 1..{} (the object maps of one env), got {}'.format(G, n_valid))
  return n_valid


def heuristic_values(method, inputs, mask=True, difference_exponent=2, weights_exponent=2, localized=False,
                     threshold=0.75, generator=None, n_valid=None):
  """Value map float64 [B, OH, OW] of one method and (optionally) the goal-overlap mask bool [B, OH, OW].

  An observation without a goal (its goal channel all zero) has `gmax = 0` (baselines.py:23): the reference divides by
  zero there, and so does the device, without a check that would need a sync: that env's values are NaN / inf and its
  action is arbitrary; the other envs of the batch are computed as ever.  An all-zero object map gives `height` 0 and a
  mask that is True everywhere (`difference` and `correlate` divide by its zero sum: NaN, as in the reference).
  A map too large to stage in one workgroup's LDS (H = 256 with h = 64) raises RuntimeError before anything is launched.

  With the grouped object maps of Stack-v2, uint8 [B, G, h, w, 1], the maps come back as [B, G, OH, OW]: row r of env b is
  what the observation (map b, object map r of env b) gives above, bit for bit; the overhead map is read where it is, not
  copied G times.  `n_valid` (ordering freedom, `env.num_maps_on_show`): only the first `n_valid` rows are computed; the
  others come back as +inf values under a False mask."""
  xm, xo = inputs
  for x in (xm, xo):
    if x.dtype != torch.uint8:    # the kernels read bytes (csrc/heuristics.hip)
      raise ValueError('heuristic_values needs uint8 observations, got {} (an env built with dtype={!r})'.format(
        x.dtype, str(x.dtype).replace('torch.', '')))
  if xm.dim() != 4 or xo.dim() not in (4, 5):
    raise ValueError('heuristic_values needs maps [B, H, W, 2] and object maps [B, h, w, 1] or [B, G, h, w, 1], got {} and {}'.format(
      tuple(xm.shape), tuple(xo.shape)))
  grouped = xo.dim() == 5
  if n_valid is not None and not grouped:
    raise ValueError('n_valid needs grouped object maps [B, G, h, w, 1]')
  if grouped:
    n_valid = _check_n_valid(n_valid, xo.shape[1])
  if not xm.is_cuda:
    raise RuntimeError('heuristic_values needs a HIP device (no CPU fallback)')
  xm = xm.contiguous(); xo = xo.contiguous()
  B, H = xm.shape[0], xm.shape[1]
  h = xo.shape[2] if grouped else xo.shape[1]
  OH = H - h + 1
  mid = METHODS[method] if isinstance(method, str) else int(method)
  if grouped:
    G = xo.shape[1]
    if xo.shape[0] != B:
      raise ValueError('{} maps but {} groups of object maps'.format(B, xo.shape[0]))
    if n_valid < G:
      vals = torch.full((B, G, OH, OH), float('inf'), dtype=torch.float64, device=xm.device)
      mk = torch.zeros((B, G, OH, OH), dtype=torch.uint8, device=xm.device) if mask else None
    else:
      vals = torch.empty((B, G, OH, OH), dtype=torch.float64, device=xm.device)
      mk = torch.empty((B, G, OH, OH), dtype=torch.uint8, device=xm.device) if mask else None
    qops.call('srl_heuristic_rows', xm, mid if mid else 2, xm, xo, vals, mk, B, G, n_valid, H, h, int(difference_exponent),
              int(weights_exponent), int(bool(localized)), float(threshold))
  else:
    vals = torch.empty((B, OH, OH), dtype=torch.float64, device=xm.device)
    mk = torch.empty((B, OH, OH), dtype=torch.uint8, device=xm.device) if mask else None
    qops.call('srl_heuristic', xm, mid if mid else 2, xm, xo, vals, mk, B, H, h, int(difference_exponent), int(weights_exponent),
              int(bool(localized)), float(threshold))
  if mid == 0:   # 'random' keeps the mask of the heuristic pass and replaces the values (all B * G maps in one draw)
    vals = torch.rand(vals.shape, generator=generator, device=xm.device, dtype=torch.float64)
  return (vals, mk.bool()) if mask else vals


def select(values, mask=None, goal=True, minorder=1, value=False, n_valid=None, chosen=False):
  """`Baseline.call` (baselines.py:201-217) on value maps float64 [B, OH, OW] (+ mask) -> actions int64 [B].

  On grouped maps [B, G, OH, OW] (Stack-v2) the same rule runs per row and the row is chosen as
  include/stackrl_baseline_rows.h defines it: actions int64 [B] = row * A + pixel; with `value` the negated maps
  [B, G, OH, OW] (rows from `n_valid` on are -inf), with `chosen` also c float64 [B, G], each row's returned value at its
  own action.  The returns are ordered (actions[, chosen][, neg])."""
  if values.dim() not in (3, 4):
    raise ValueError('select needs value maps [B, OH, OW] or [B, G, OH, OW], got {}'.format(tuple(values.shape)))
  grouped = values.dim() == 4
  if (n_valid is not None or chosen) and not grouped:
    raise ValueError('n_valid and chosen need grouped value maps [B, G, OH, OW]')
  values = values.contiguous()
  B, OH = values.shape[0], values.shape[2 if grouped else 1]
  mk = mask.to(torch.uint8).contiguous() if (goal and mask is not None) else None
  if goal and mk is None:
    raise ValueError('goal=True needs the goal-overlap mask')
  if grouped and mk is not None and mk.shape != values.shape:
    raise ValueError('mask {} does not match the values {}'.format(tuple(mk.shape), tuple(values.shape)))
  actions = torch.empty(B, dtype=torch.int64, device=values.device)
  neg = torch.empty_like(values) if value else None
  if grouped:
    G = values.shape[1]
    n_valid = _check_n_valid(n_valid, G)
    c = torch.empty((B, G), dtype=torch.float64, device=values.device) if chosen else None
    qops.call('srl_baseline_rows_select', values, values, mk, int(bool(goal)), int(minorder), B, G, n_valid, OH, actions, c, neg)
    out = (actions,) + ((c,) if chosen else ()) + ((neg,) if value else ())
    return out if len(out) > 1 else actions
  qops.call('srl_baseline_select', values, values, mk, int(bool(goal)), int(minorder), actions, neg, B, OH)
  return (actions, neg) if value else actions


def _minimum_filter_const0(v, size):
  """scipy.ndimage.minimum_filter(v, size=size, mode='constant') (0 outside the array), in numpy."""
  r = size // 2
  p = np.pad(v, r, mode='constant', constant_values=0.0)
  return np.lib.stride_tricks.sliding_window_view(p, (size, size)).min(axis=(2, 3))


def baseline_rows_reference(values, mask, goal=True, minorder=1, n_valid=None):
  """The selection of include/stackrl_baseline_rows.h in numpy float64 on the CPU: what the reference's
  `Baseline(batched=True, batchwise=True)` does with the value maps of one env's rows (`Baseline.call`, baselines.py:201-217,
  per row; `PyGreedy.__call__`, agents/policies.py:57-91, over the rows).

  values float64 [B, G, OH, OW] and mask bool of the same shape (numpy arrays or torch tensors; the mask may be None with
  `goal=False`) -> (actions int64 [B] = row * A + pixel, chosen float64 [B, G], neg float64 [B, G, OH, OW]) as numpy arrays.
  Rows from `n_valid` on are not read; their `chosen` and `neg` are -inf."""
  values = np.asarray(values.detach().cpu() if isinstance(values, torch.Tensor) else values, dtype=np.float64)
  if mask is not None:
    mask = np.asarray(mask.detach().cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
  if values.ndim != 4:
    raise ValueError('baseline_rows_reference needs value maps [B, G, OH, OW], got {}'.format(values.shape))
  if goal and mask is None:
    raise ValueError('goal=True needs the goal-overlap mask')
  if mask is not None and mask.shape != values.shape:
    raise ValueError('mask {} does not match the values {}'.format(mask.shape, values.shape))
  if int(minorder) < 0:
    raise ValueError('minorder must not be negative')
  B, G = values.shape[:2]
  A = values.shape[2] * values.shape[3]
  n_valid = _check_n_valid(n_valid, G)
  actions = np.zeros(B, np.int64)
  chosen = np.full((B, G), -np.inf)
  neg = np.full(values.shape, -np.inf)
  for b in range(B):
    acts = []
    for r in range(n_valid):
      v = values[b, r]
      if goal:
        m = mask[b, r]
        cand = m
        if minorder:
          minima = np.logical_and(m, _minimum_filter_const0(v, 1 + 2 * int(minorder)) == v)
          if np.any(minima):
            cand = minima
        a = int(np.argmin(np.where(cand, v, np.inf)))
        neg[b, r] = -np.where(m, v, (v[m].max() if m.any() else -np.inf) + 0.001)
      else:
        a = int(np.argmin(v))
        neg[b, r] = -v
      acts.append(a)
      chosen[b, r] = neg[b, r].flat[a]
    row = int(np.argmax(chosen[b, :n_valid]))      # ties to the first row (policies.py:79)
    actions[b] = row * A + acts[row]
  return actions, chosen, neg


class Baseline(object):
  """stackrl.Baseline (baselines.py:168-217)."""

  def __init__(self, method='random', goal=True, minorder=1, value=False, seed=None, **kwargs):
    if isinstance(method, str):
      if method not in METHODS:
        raise ValueError('Invalid value {} for argument method. Must be in {}'.format(method, list(METHODS)))   # :184-187
    else:
      raise TypeError('Invalid type {} for argument method.'.format(type(method)))
    self.method, self.goal, self.minorder, self.value, self.kwargs = method, goal, minorder, value, kwargs
    self._seed, self._gen = seed, None

  def __call__(self, inputs, n_valid=None):
    """Observations ([B, H, W, 2], [B, h, w, 1]) -> actions [B] (and the negated maps [B, OH, OW] with `value=True`).

    The grouped observation of Stack-v2, object maps [B, G, h, w, 1]: the reference's `batched=True, batchwise=True` per env
    (include/stackrl_baseline_rows.h) -> actions [B] = row * A + pixel, the action `VecStackEnv` takes, and with `value=True`
    the negated maps as [B, G * A], rows from `n_valid` (`env.num_maps_on_show` under ordering freedom) on at -inf: the call
    signature of `policies.OrientationGreedy` / `FusedOrientationGreedy`."""
    if self.method == 'random' and self._gen is None:
      self._gen = torch.Generator(device=inputs[0].device)
      if self._seed is not None:
        self._gen.manual_seed(int(self._seed))
    kw = {k: v for k, v in self.kwargs.items() if k in ('difference_exponent', 'weights_exponent', 'localized', 'threshold')}
    grouped = inputs[1].dim() == 5
    if grouped:
      kw['n_valid'] = n_valid
    elif n_valid is not None:
      raise ValueError('n_valid needs grouped object maps [B, G, h, w, 1]')
    out = heuristic_values(self.method, inputs, mask=self.goal, generator=self._gen, **kw)
    vals, mk = out if self.goal else (out, None)
    if not grouped:
      return select(vals, mk, goal=self.goal, minorder=self.minorder, value=self.value)
    out = select(vals, mk, goal=self.goal, minorder=self.minorder, value=self.value, n_valid=n_valid)
    return (out[0], out[1].reshape(out[1].shape[0], -1)) if self.value else out
