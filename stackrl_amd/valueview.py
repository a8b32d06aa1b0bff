"""The frames of a visualised comparison run, drawn on the device: what the reference's `run(..., visualize=True)`
(`stackrl/test.py:230-317`) shows in a matplotlib figure at every step — the overhead view, the object view and every
policy's value map in `viridis`, each map scaled by itself, the driving policy's framed in yellow — as uint8 images made by
libstackrl_valueview.so (include/stackrl_valueview.h states the definition, csrc/valueview.hip holds the two kernels,
tests/value_view_cases.py the numpy restatement).

`ValueView.frames` draws the envs asked for from `env.render('rgb_array', dtype='uint8')` and the policies' maps where they
lie; `Recorder` is the callable `compare.run(..., visualize=...)` takes; `write_ppm` writes one frame."""
import ctypes
import os

import numpy as np
import torch

from stackrl_amd import _bind

MAX_POLICIES = 8
MAX_SCALE = 8

_VP, _I32, _INT = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int
# export -> (restype, argtypes, error accessor or None): every declaration of include/stackrl_valueview.h (pointers as void*);
# tests/test_abi.py holds the table to the header and the library.
_SIGS = {
  'srl_valueview_layout': (_INT, [_I32] * 4 + [_VP], 'srl_valueview_last_error'),
  'srl_valueview_window': (_INT, [_I32, _I32, _VP], 'srl_valueview_last_error'),
  'srl_valueview_lut': (_INT, [_VP], 'srl_valueview_last_error'),
  'srl_valueview_frames': (_INT, [_I32] + [_VP] * 8 + [_I32] * 5 + [_VP] * 4 + [_I32] * 4 + [_VP] * 3, 'srl_valueview_last_error'),
  'srl_valueview_last_error': (ctypes.c_char_p, [], None),
  'srl_valueview_build_info': (ctypes.c_char_p, [], None),
}

load, call = _bind.binding('valueview', _SIGS)


def _host(name, *args):
  lib = load()
  if getattr(lib, name)(*args):
    raise ValueError(lib.srl_valueview_last_error().decode())


def layout(H, h, P, scale):
  """The layout of a frame (`srl_valueview_layout`): a dict of FH, FW, nv, ncol, nline, TB."""
  out = (ctypes.c_int32 * 8)()
  _host('srl_valueview_layout', int(H), int(h), int(P), int(scale), out)
  return dict(zip(('FH', 'FW', 'nv', 'ncol', 'nline', 'TB'), out[:6]))


def window(P, index):
  """The first policy shown when policy `index` of P drives (`srl_valueview_window`); tile k shows policy window + k."""
  out = ctypes.c_int32(-1)
  _host('srl_valueview_window', int(P), int(index), ctypes.byref(out))
  return out.value


def lut():
  """The colour table the kernels use, uint8 [256, 3] (`srl_valueview_lut`)."""
  out = (ctypes.c_uint8 * 768)()
  _host('srl_valueview_lut', out)
  return np.frombuffer(out, dtype=np.uint8).reshape(256, 3).copy()


def tile_order(names, index):
  """The names of the policies the tiles of a frame show, in tile order, when policy `index` drives."""
  names = list(names)
  first = window(len(names), index)
  return names[first:first + layout(1, 1, len(names), 1)['nv']]


class ValueView(object):
  """Frames of `scale` output pixels per source pixel; `mark` also draws each policy's chosen pixel in its tile and the window
  of the driving policy's in the overhead view, in red (not in the reference)."""

  def __init__(self, scale=2, mark=False):
    self.scale, self.mark = int(scale), bool(mark)
    if not 1 <= self.scale <= MAX_SCALE:
      raise ValueError('scale must be in 1..{}, got {}'.format(MAX_SCALE, scale))
    self._scratch = None

  def frames(self, rgb0, rgb1, values, actions=None, index=0, indexes=None, out=None):
    """uint8 [n, FH, FW, 3] on the device of `rgb0`, one frame per env of `indexes` (default: every env, in order; an int
    tensor or a sequence, repeats allowed, clamped to 0..B-1).  rgb0 uint8 [B, H, H, 3] and rgb1 uint8 [B, h, h, 3]: what
    `env.render('rgb_array', dtype='uint8')` returns.  values, actions: what `compare.MapStatistics.step` takes — P maps
    [B, A] or [B, G * A], float32 or float64 (another float type is converted to float32), and None or P tensors [B] =
    row * A + pixel, which maps of several rows need.  index: the driving policy.  Two launches on the current stream;
    nothing is synchronised."""
    if not (isinstance(rgb0, torch.Tensor) and rgb0.is_cuda):
      raise RuntimeError('ValueView.frames needs the images on a HIP device')
    dev = rgb0.device
    if rgb0.dim() != 4 or rgb1.dim() != 4 or rgb0.shape[0] != rgb1.shape[0] or rgb0.shape[1] != rgb0.shape[2] or \
       rgb1.shape[1] != rgb1.shape[2] or rgb0.shape[3] != 3 or rgb1.shape[3] != 3:
      raise ValueError('the images must be [B, H, H, 3] and [B, h, h, 3], got {} and {}'.format(tuple(rgb0.shape), tuple(rgb1.shape)))
    if rgb0.dtype != torch.uint8 or rgb1.dtype != torch.uint8 or rgb1.device != dev:
      raise ValueError("the images must be uint8 on one device: render('rgb_array', dtype='uint8')")
    rgb0, rgb1 = rgb0.contiguous(), rgb1.contiguous()
    B, H, h = int(rgb0.shape[0]), int(rgb0.shape[1]), int(rgb1.shape[1])
    values = list(values)
    P = len(values)
    if not 1 <= P <= MAX_POLICIES:
      raise ValueError('the number of policies must be in 1..{}, got {}'.format(MAX_POLICIES, P))
    A = (H - h + 1) ** 2
    maps = []
    for v in values:
      if v.device != dev:
        raise ValueError('map on {}, the images on {}'.format(v.device, dev))
      if v.shape[0] != B or v.numel() != values[0].numel() or v.numel() % (B * A):
        raise ValueError('maps must be [B, A] or, with actions, [B, G * A]: got {} for B = {}, A = {}'.format(tuple(v.shape), B, A))
      if v.dtype not in (torch.float32, torch.float64):
        v = v.float()
      maps.append(v.contiguous())
    G = maps[0].numel() // (B * A)
    if G > 1 and actions is None:
      raise ValueError('maps of {} rows per env need the actions that choose the row'.format(G))
    if actions is not None:
      actions = list(actions)
      if len(actions) != P or any(tuple(a.shape) != (B,) for a in actions):
        raise ValueError('actions must be {} tensors [{}]'.format(P, B))
      actions = torch.stack([a.to(device=dev, dtype=torch.int64) for a in actions]).contiguous()
    if indexes is None:
      indexes = torch.arange(B, dtype=torch.int32, device=dev)
    else:
      indexes = torch.as_tensor(indexes).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    n = int(indexes.shape[0])
    l = layout(H, h, P, self.scale)
    shape = (n, l['FH'], l['FW'], 3)
    if out is None:
      out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
      raise ValueError('out must be a contiguous uint8 tensor {} on {}'.format(shape, dev))
    if self._scratch is None or self._scratch.device != dev or self._scratch.numel() < P * max(n, 1) * 2:
      self._scratch = torch.empty(P * max(n, 1) * 2, dtype=torch.float32, device=dev)
    mask = sum(1 << j for j, v in enumerate(maps) if v.dtype == torch.float64)
    call('srl_valueview_frames', rgb0, P, *(maps + [None] * (MAX_POLICIES - P)), mask, B, G, H, h, rgb0, rgb1, actions, indexes,
         n, int(index), self.scale, int(self.mark), self._scratch, out)
    return out


def write_ppm(path, image):
  """One frame, uint8 [rows, columns, 3] (a tensor or an array), as a binary PPM file."""
  if isinstance(image, torch.Tensor):
    image = image.detach().cpu().numpy()
  image = np.ascontiguousarray(image)
  if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
    raise ValueError('write_ppm needs a uint8 image [rows, columns, 3], got {} {}'.format(image.dtype, image.shape))
  with open(path, 'wb') as f:
    f.write('P6\n{} {}\n255\n'.format(image.shape[1], image.shape[0]).encode())
    f.write(image.tobytes())


class Recorder(object):
  """The standard `visualize` of `compare.run`: keeps the frames of the envs `envs`, writes each as
  `<dirname>/policy<p>_step<t>_env<i>.ppm`, and `close()` — which `run` calls at its end — writes them all as
  `<dirname>/frames.npy`, uint8 [P, num_steps, len(envs), FH, FW, 3] in the order they came.  `run` reads `view` (the
  `ValueView` that draws) and `envs` off the callable it is given; one without them gets `ValueView()` and every env."""

  def __init__(self, dirname, envs=(0,), scale=2, mark=False):
    self.dirname = dirname
    self.envs = tuple(int(e) for e in envs)
    self.view = ValueView(scale=scale, mark=mark)
    self.frames = []            # (step, policy, uint8 [len(envs), FH, FW, 3] on the host)

  def __call__(self, step, policy_index, frames):
    if not os.path.isdir(self.dirname):
      os.makedirs(self.dirname)
    frames = frames.cpu().numpy()
    self.frames.append((int(step), int(policy_index), frames))
    for e, frame in zip(self.envs, frames):
      write_ppm(os.path.join(self.dirname, 'policy{}_step{}_env{}.ppm'.format(int(policy_index), int(step), e)), frame)

  def stacked(self):
    """uint8 [P, num_steps, len(envs), FH, FW, 3] of the frames so far (whole policies)."""
    policies = sorted({p for _, p, _ in self.frames})
    per = [np.stack([f for _, q, f in self.frames if q == p]) for p in policies]
    steps = min(len(x) for x in per)
    return np.stack([x[:steps] for x in per])

  def close(self):
    if self.frames:
      np.save(os.path.join(self.dirname, 'frames.npy'), self.stacked())
