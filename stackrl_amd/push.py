"""Push test: does the pile stand?  Fork it, give its rocks a velocity increment, let it move, measure how far every rock
went — all on the device (`srl_poses`, `srl_kick`, `srl_pose_distances`; include/stackrl_hip.h "Push test").

`PoseDistances` is what `VecStackEnv.distances` and `VecStackEnv.push` return: per body slot the translation and rotation
error against a reference pose, the height change and the speed, and a summary per env, as device tensors with named views.
`PushSpec` says how hard, how long and in which directions to push; `PushTest(env, trials=k)` holds a scratch env of B x k
envs like `Lookahead`'s, and `evaluate` pushes k forks of every pile without touching `env`."""
import math

import torch

ROW_WORDS = 4         # perr, oerr, dz, speed
SUMMARY_WORDS = 8     # nb, moved, max_perr, max_oerr, sum_perr, min_dz, max_speed, max_spin
KICK_ALL, KICK_LAST = -1, -2          # SRL_KICK_ALL, SRL_KICK_LAST
_ROW = {'perr': 0, 'oerr': 1, 'dz': 2, 'speed': 3}
_SUMMARY = {'nb': 0, 'moved': 1, 'max_perr': 2, 'max_oerr': 3, 'sum_perr': 4, 'min_dz': 5, 'max_speed': 6, 'max_spin': 7}
MODES = ('bump', 'shake', 'last')


def default_tol(config):
  """(tol_p, tol_o) of "moved" where none is given: one pixel of the maps, object_max_dimension / object_res metres, and the
  angle by which a point at half the largest rock dimension from the axis travels one pixel, 2 / object_res radians —
  below both, neither map can show the difference."""
  return float(config.object_max_dimension) / float(config.object_res), 2.0 / float(config.object_res)


def select_code(select):
  """`select` of `kick` -> the export's code: 'all', 'last' or a body slot (the export refuses one outside 0 .. L - 1)."""
  if select == 'all':
    return KICK_ALL
  if select == 'last':
    return KICK_LAST
  if isinstance(select, str) or isinstance(select, bool):
    raise ValueError("select must be 'all', 'last' or a body slot, got {!r}".format(select))
  s = int(select)
  if s < 0:
    raise ValueError("select must be 'all', 'last' or a body slot, got {!r}".format(select))
  return s


def increments(dv, B, L, device):
  """`dv` of `kick` as the export reads it: (contiguous float32 [B, 8] or [B, L, 8] on `device`, per_body).  `dv` may be
  [B, 8], [B, L, 8] (linear increment in columns 0 - 2, angular in 4 - 6) or [B, 3], [B, L, 3] (linear only)."""
  dv = torch.as_tensor(dv).to(device=device, dtype=torch.float32)
  shape = tuple(dv.shape)
  if shape not in ((B, 8), (B, 3), (B, L, 8), (B, L, 3)):
    raise ValueError('dv must have shape [{B}, 8], [{B}, 3], [{B}, {L}, 8] or [{B}, {L}, 3], got {s}'.format(B=B, L=L, s=list(shape)))
  if shape[-1] == 3:
    wide = torch.zeros(shape[:-1] + (8,), dtype=torch.float32, device=device)
    wide[..., 0:3] = dv
    dv = wide
  return dv.contiguous(), int(dv.dim() == 3)


class PoseDistances(object):
  """rows float32 [..., L, 4] (perr, oerr, dz, speed per body slot, zeros at or above the env's body count) and summary
  float32 [..., 8] per env; the leading dimensions are [B], or [B, k] from `PushTest`.  Views of the rows: `perr` (metres),
  `oerr` (radians), `dz`, `speed`; of the summary: `nb`, `moved` (bodies beyond a tolerance, a NaN included), `max_perr`,
  `max_oerr`, `sum_perr`, `min_dz`, `max_speed`, `max_spin`.  `at_rest`: the stop criterion of `Simulator.step`
  (simulator.py:328-335), no body faster than `velocity_threshold`."""

  def __init__(self, rows, summary, velocity_threshold):
    self.rows, self.summary, self.velocity_threshold = rows, summary, float(velocity_threshold)

  def __getattr__(self, name):
    if name in _ROW:
      return self.rows[..., _ROW[name]]
    if name in _SUMMARY:
      return self.summary[..., _SUMMARY[name]]
    raise AttributeError(name)

  @property
  def at_rest(self):
    return self.max_speed <= self.velocity_threshold

  @property
  def moved_fraction(self):
    """moved / nb, 0 for an env without a body."""
    return self.moved / torch.clamp(self.nb, min=1.0)

  def reshape(self, *lead):
    return PoseDistances(self.rows.reshape(tuple(lead) + tuple(self.rows.shape[-2:])), self.summary.reshape(tuple(lead) + (SUMMARY_WORDS,)),
                         self.velocity_threshold)

  def cpu(self):
    return PoseDistances(self.rows.cpu(), self.summary.cpu(), self.velocity_threshold)

  def __len__(self):
    return int(self.summary.shape[0])


def empty(B, L, device, velocity_threshold):
  """Uninitialised tensors for `srl_pose_distances` to fill."""
  return PoseDistances(torch.empty((B, L, ROW_WORDS), dtype=torch.float32, device=device),
                       torch.empty((B, SUMMARY_WORDS), dtype=torch.float32, device=device), velocity_threshold)


def check_tensors(what, wanted, device):
  """Every (tensor, shape, dtype) of `wanted` is a contiguous tensor of that shape and type on `device`."""
  for t, shape, dt in wanted:
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dt or t.device != device or not t.is_contiguous():
      raise ValueError('{} must be contiguous tensors on {}: {}'.format(
        what, device, ', '.join('{} {}'.format(d, list(s)) for _, s, d in wanted)))


class PushSpec(object):
  """How to push: `speed` (m/s) of the horizontal velocity increment, `substeps` to let the pile move, `mode`, the
  tolerances `tol` = (metres, radians) of "moved" (None: `default_tol`) and the `seed` of the directions.
    'bump'   one direction per env and trial for every rock: what the pile sees when the ground suddenly moves the other way
    'shake'  a direction of its own for every rock
    'last'   one direction per env and trial, for the last placed rock only"""

  def __init__(self, speed=0.1, substeps=50, mode='bump', tol=None, seed=0):
    if mode not in MODES:
      raise ValueError('mode must be one of {}, got {!r}'.format(MODES, mode))
    if int(substeps) < 1:
      raise ValueError('substeps must be at least 1')
    self.speed, self.substeps, self.mode, self.seed = float(speed), int(substeps), mode, int(seed)
    self.tol = None if tol is None else (float(tol[0]), float(tol[1]))

  @property
  def select(self):
    return 'last' if self.mode == 'last' else 'all'

  def draw(self, B, k, L, device):
    """dv float32 [B, k, 8] ('bump', 'last') or [B, k, L, 8] ('shake') on `device`: speed (cos t, sin t, 0) with t = 2 pi u,
    u uniform in [0, 1) from a `torch.Generator` seeded with `seed` — the same draw for the same (seed, B, k, L, mode)."""
    gen = torch.Generator(device='cpu')
    gen.manual_seed(self.seed)
    shape = (B, k, L) if self.mode == 'shake' else (B, k)
    theta = (2.0 * math.pi) * torch.rand(shape, generator=gen, dtype=torch.float64)
    dv = torch.zeros(shape + (8,), dtype=torch.float32)
    dv[..., 0] = (self.speed * torch.cos(theta)).to(torch.float32)
    dv[..., 1] = (self.speed * torch.sin(theta)).to(torch.float32)
    return dv.to(device)


class PushTest(object):
  """`PushTest(env, trials=k)`: k pushes of a fork of every pile of `env` (a `VecStackEnv`, `PipelinedVecStackEnv` or
  `StartedVecStackEnv` of B envs), on a scratch `VecStackEnv` of B x k envs built as `Lookahead` builds its own.  kwargs go to
  the scratch env's constructor."""

  def __init__(self, env, trials=1, **kwargs):
    from stackrl_amd.lookahead import Lookahead
    self._fork = Lookahead(env, trials, **kwargs)     # the scratch env, the signature check, `_follow_pool`, the fork itself
    self.env, self.k, self.B = env, self._fork.k, self._fork.B
    self.scratch = self._fork.scratch

  def close(self):
    self._fork.close()

  def evaluate(self, spec_or_dv, substeps=None, select='all', tol=None):
    """A `PushSpec`, or increments `dv` [B, k, 8 | 3] / [B, k, L, 8 | 3] with `substeps`, `select` and `tol` -> the
    `PoseDistances` of the B x k pushed forks, [B, k, ...], measured from the poses before the push.  `env` is not touched: its
    records are gathered (csrc/state.hip), written k-fold into the scratch handle and pushed there in place."""
    s, B, k = self.scratch, self.B, self.k
    L = s.config.episode_length
    if isinstance(spec_or_dv, PushSpec):
      spec = spec_or_dv
      dv, substeps, select, tol = spec.draw(B, k, L, s._device), spec.substeps, spec.select, spec.tol
    else:
      dv = torch.as_tensor(spec_or_dv)
      if substeps is None:
        raise ValueError('increments need substeps')
    if tuple(dv.shape[:2]) != (B, k) or dv.dim() not in (3, 4):
      raise ValueError('dv must have shape [{}, {}, 8 | 3] or [{}, {}, {}, 8 | 3], got {}'.format(B, k, B, k, L, list(dv.shape)))
    self._fork.fork()
    out = s.push(dv.reshape((B * k,) + tuple(dv.shape[2:])), substeps, select=select, tol=tol)
    return out.reshape(B, k)
