"""The procedural rock generator on the device: `stackrl/envs/data/generator.py`'s `box` recipe and `generate` (what
`assets.generate_rock` restates on scipy, one rock at a time) as one launch of libstackrl_rocks.so per batch of rocks
(include/stackrl_rocks.h states the definition, csrc/rocks.hip is the kernel, tests/rocks_cases.py the numpy restatement).

`generate` returns a `RockBatch` of device tensors; `RockBatch.to_pool` compacts it into an `assets.MeshPool`, which
`VecStackEnv.set_pool` loads into a live env; `generate_pool` makes the families of `assets.generate_pool`."""
import ctypes
import dataclasses
import os

import numpy as np
import torch

from stackrl_amd import _bind
from stackrl_amd import assets as _assets
from stackrl_amd.config import MAX_TRIS, MAX_VERTS

MAX_POINTS = 386
OK, OVERFLOW, DEGENERATE = 0, 1, 2
TAG = 0x524f434b              # the second word of the Philox key (include/stackrl_rocks.h)
DENSITY_DRAW = 0xffffffff


class Params(ctypes.Structure):
  """`srl_rocks_params`."""
  _fields_ = [('radius', ctypes.c_float), ('irregularity', ctypes.c_float), ('extents', ctypes.c_float * 3),
              ('subdivisions', ctypes.c_int32), ('density_lo', ctypes.c_float), ('density_hi', ctypes.c_float),
              ('fit', ctypes.c_int32), ('seed', ctypes.c_uint32)]


_VP, _I32, _I64, _INT = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int
# export -> (restype, argtypes, error accessor or None): every declaration of include/stackrl_rocks.h (pointers as void*);
# tests/test_abi.py holds the table to the header and the library.
_SIGS = {
  'srl_rocks_points': (_INT, [_I32, _VP], None),
  'srl_rocks_generate': (_INT, [_VP, _I64, _I32, _VP, _I32] + [_VP] * 11, 'srl_rocks_last_error'),
  'srl_rocks_last_error': (ctypes.c_char_p, [], None),
  'srl_rocks_build_info': (ctypes.c_char_p, [], None),
}

load, call = _bind.binding('rocks', _SIGS)


def n_points(subdivisions):
  """8 / 26 / 98 / 386 points for 0..3 subdivisions (`srl_rocks_points`, without the library)."""
  s = int(subdivisions)
  if not 0 <= s <= 3:
    raise ValueError('subdivisions must be in 0..3, got {}'.format(subdivisions))
  return (8, 26, 98, 386)[s]


@dataclasses.dataclass
class RockBatch:
  """What one `srl_rocks_generate` call wrote, as device tensors (rows beyond a rock's counts are zero, -1 in `vert_src`)."""
  verts: torch.Tensor      # float32 [n, MAX_VERTS, 3]
  vert_src: torch.Tensor   # int32 [n, MAX_VERTS]: the input point each vertex is
  tris: torch.Tensor       # int32 [n, MAX_TRIS, 3], local, outward CCW
  counts: torch.Tensor     # int32 [n, 2] = nv, nt
  mass_com: torch.Tensor   # float32 [n, 4]
  inertia: torch.Tensor    # float32 [n, 6] ixx ixy ixz iyy iyz izz about the centre of mass
  xform: torch.Tensor      # float32 [n, 13]: s, R, c with final = s R (point - c)
  metrics: torch.Tensor    # float32 [n, 4]: volume, rectangularity, aspect ratio, OBB volume
  status: torch.Tensor     # int32 [n]: 0 ok, 1 overflow, 2 degenerate
  points: object           # float32 [n, P, 3] (`return_points`) or None
  params: dict             # radius, irregularity, extents, subdivisions, density, fit, seed
  first_index: int

  def __len__(self):
    return int(self.status.shape[0])

  def meshes(self):
    """[(verts, tris, mass_com)] in numpy, one per rock.  A rock whose status is not 0 is finished on the host from its own
    points (`finish_on_host`), which needs `return_points=True`."""
    status = self.status.cpu().numpy()
    counts = self.counts.cpu().numpy()
    verts, tris, mc = self.verts.cpu().numpy(), self.tris.cpu().numpy(), self.mass_com.cpu().numpy()
    out = []
    for i in range(len(status)):
      if status[i] == OK:
        nv, nt = counts[i]
        out.append((verts[i, :nv].copy(), tris[i, :nt].copy(), mc[i].copy()))
      else:
        if self.points is None:
          raise ValueError('rock {} has status {}: finishing it on the host needs return_points=True'.format(i, status[i]))
        out.append(finish_on_host(self.points[i].cpu().numpy(), self.first_index + i, **self.params)[:3])
    return out

  def to_pool(self, names=None):
    """The batch as an `assets.MeshPool` (names default to the global rock indexes)."""
    names = list(names) if names is not None else [str(self.first_index + i) for i in range(len(self))]
    if len(names) != len(self):
      raise ValueError('{} names for {} rocks'.format(len(names), len(self)))
    return _assets.pack(self.meshes(), names)


def density_of(index, seed, density=(2200., 2600.)):
  """The density of rock `index` under `seed`: the fixed draw of its stream (include/stackrl_rocks.h)."""
  from stackrl_amd.dqn import philox4x32_10
  index = int(index) % 2 ** 64
  x = int(philox4x32_10(torch.tensor([index & 0xffffffff, index >> 32, DENSITY_DRAW, 0], dtype=torch.int64),
                        torch.tensor([int(seed) % 2 ** 32, TAG], dtype=torch.int64))[0])
  lo, hi = float(np.float32(density[0])), float(np.float32(density[1]))
  return lo + (x + 0.5) * 2.0 ** -32 * (hi - lo)


def finish_on_host(points, index, radius=0.0625, density=(2200., 2600.), fit=0, seed=0, **_):
  """Stages 2-5 for one rock on the host, through `assets.hull_mesh`, `mass_properties` and `oriented_bounds` (what
  `assets.generate_rock` does after the noise): (verts float32, tris int32, mass_com float32 [4], scale)."""
  v, t = _assets.hull_mesh(np.asarray(points, dtype=np.float64))
  _, com = _assets.mass_properties(v, t)
  v = v - com
  R, centre, ext = _assets.oriented_bounds(v, t)
  factor = radius / np.linalg.norm(v, axis=1).max() if fit == 0 else 2 * radius / ext.max()
  factor = min(1.0, factor)
  v = ((v - centre) @ R.T) * factor
  v = v @ np.array([[0., 0, -1], [0, 1, 0], [1, 0, 0]])
  v = v.astype(np.float32)
  volume, c = _assets.mass_properties(v.astype(np.float64), t)
  rho = density_of(index, seed, density)
  return v, t.astype(np.int32), np.array([rho * volume, c[0], c[1], c[2]], dtype=np.float32), factor


def generate(n, irregularity=0.5, seed=None, first_index=0, radius=0.0625, extents=(1., 1 / 2, 1 / 3), subdivisions=3,
             density=(2200., 2600.), fit=0, points=None, return_points=False, device=None):
  """Rocks `first_index .. first_index + n - 1` of the stream `seed` on `device` (default: the current HIP device), one
  launch on the current stream; nothing is synchronised.  Rock `first_index + i` is the same rock whatever the batch it is
  made in.  `points`: a float32 tensor [n, P, 3] (P in 4..386) to take the hulls of instead of making the noisy points.
  `seed=None` draws one from the operating system.  Returns a `RockBatch`."""
  if not torch.cuda.is_available():
    raise RuntimeError('rocks.generate needs a HIP device: the host path is assets.generate_rock')
  n = int(n)
  if seed is None:
    seed = int.from_bytes(os.urandom(4), 'little')
  if points is not None:
    points = torch.as_tensor(points)
    if device is None and points.is_cuda:
      device = points.device
  device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
  if device.index is None:
    device = torch.device('cuda', torch.cuda.current_device())
  if points is not None:
    points = points.to(device=device, dtype=torch.float32).contiguous()
    if points.dim() != 3 or points.shape[0] != n or points.shape[2] != 3:
      raise ValueError('points must be [n, P, 3], got {}'.format(tuple(points.shape)))
    P = int(points.shape[1])
  else:
    P = n_points(subdivisions)
  par = Params(float(radius), float(irregularity), (ctypes.c_float * 3)(*[float(e) for e in extents]), int(subdivisions),
               float(density[0]), float(density[1]), int(fit), int(seed) % 2 ** 32)
  rows = max(n, 1)

  def new(shape, dtype):
    return torch.zeros((rows,) + shape, dtype=dtype, device=device)
  b = RockBatch(new((MAX_VERTS, 3), torch.float32), new((MAX_VERTS,), torch.int32), new((MAX_TRIS, 3), torch.int32),
                new((2,), torch.int32), new((4,), torch.float32), new((6,), torch.float32), new((13,), torch.float32),
                new((4,), torch.float32), new((), torch.int32),
                (points if points is not None else new((P, 3), torch.float32)) if return_points else None,
                dict(radius=float(radius), irregularity=float(irregularity), extents=tuple(float(e) for e in extents),
                     subdivisions=int(subdivisions), density=(float(density[0]), float(density[1])), fit=int(fit),
                     seed=int(seed) % 2 ** 32), int(first_index))
  call('srl_rocks_generate', b.status, ctypes.byref(par), int(first_index), n, points, P if points is not None else 0,
       b.points if (return_points and points is None) else None, b.verts, b.vert_src, b.tris, b.counts, b.mass_com,
       b.inertia, b.xform, b.metrics, b.status)
  return b


def family_names(n, irregularities):
  """(irregularity, name) per rock, in the order and with the names of `assets.generate_pool`."""
  per = max(1, n // len(irregularities))
  out = []
  for irr in irregularities:
    for k in range(per):
      if len(out) >= n:
        break
      out.append((irr, '{}_{:03d}'.format(int(round(irr * 100)), k)))
  return out


def generate_pool(n=5000, seed=11, irregularities=None, device=None, **kwargs):
  """The families and names of `assets.generate_pool` ('50_000' ...: ten families, irregularity 0.50 .. 0.95, `n // 10`
  rocks each) made on the device: one launch per family, rock k of the pool is rock k of the stream `seed`.  A rock the
  kernel does not report ok is finished on the host from its own points, so the pool is complete and the same on every run.
  `kwargs`: the other arguments of `generate`."""
  if irregularities is None:
    irregularities = [i / 100. for i in range(50, 100, 5)]
  rocks = family_names(int(n), list(irregularities))
  meshes, start = [], 0
  batches = []
  while start < len(rocks):                      # launch every family, then read back
    stop = start
    while stop < len(rocks) and rocks[stop][0] == rocks[start][0]:
      stop += 1
    batches.append(generate(stop - start, rocks[start][0], seed=seed, first_index=start, return_points=True, device=device,
                            **kwargs))
    start = stop
  for b in batches:
    meshes += b.meshes()
  return _assets.pack(meshes, [name for _, name in rocks])
