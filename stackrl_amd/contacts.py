"""Contact points of every env's pile (`srl_contact_points`, include/stackrl_hip.h "Contact points"): the reference's
`Simulator.contact_points` (simulator.py:131-133, pybullet's `getContactPoints`) for a batch, as device tensors.

`ContactPoints` is what `VecStackEnv.contact_points` returns: per env the number of contacts, the two body slots of each
(-1 = the ground) and a row of float32 words per contact, with named views of the row's parts; optionally the net contact
force and torque on every body."""
import collections

import torch

# the words of a row (include/stackrl_hip.h): name -> (first word, words)
FIELDS = collections.OrderedDict([
  ('position_on_a', (0, 3)), ('position_on_b', (3, 3)), ('normal_on_b', (6, 3)), ('distance', (9, 1)),
  ('normal_force', (10, 1)), ('lateral_friction1', (11, 1)), ('lateral_friction_dir1', (12, 3)),
  ('lateral_friction2', (15, 1)), ('lateral_friction_dir2', (16, 3))])
ROW_WORDS = 20        # srl_contact_row_words(): the fields above and a word that is 0
WRENCH_WORDS = 8      # force xyz, number of points, torque about the body's position xyz, 0
CONTACT_FLAG = 0      # getContactPoints' first field ("reserved") and its two link indexes (-1: the base) are constants
LINK_INDEX = -1


class ContactPoints(object):
  """count int32 [B]: the contacts of each env (all of them, or the last placed rock's), whatever the capacity C;
  bodies int32 [B, C, 2]: body slots (a, b), b = -1 for the ground; rows float32 [B, C, ROW_WORDS];
  wrench float32 [B, L, 8] or None.  Only the first min(count, C) rows of an env are written."""

  def __init__(self, count, bodies, rows, wrench=None):
    self.count, self.bodies, self.rows, self.wrench = count, bodies, rows, wrench

  @property
  def capacity(self):
    return int(self.rows.shape[1])

  @property
  def overflowed(self):
    """bool [B]: the env has more contacts than rows were given."""
    return self.count > self.capacity

  @property
  def body_a(self):
    return self.bodies[..., 0]

  @property
  def body_b(self):
    return self.bodies[..., 1]

  def _field(self, name):
    o, n = FIELDS[name]
    return self.rows[..., o] if n == 1 else self.rows[..., o:o + n]

  def __getattr__(self, name):        # the named views of `rows`: position_on_a [B, C, 3], distance [B, C], ...
    if name in FIELDS:
      return self._field(name)
    raise AttributeError(name)

  @property
  def net_force(self):
    return None if self.wrench is None else self.wrench[..., 0:3]

  @property
  def net_torque(self):
    return None if self.wrench is None else self.wrench[..., 4:7]

  def cpu(self):
    return ContactPoints(self.count.cpu(), self.bodies.cpu(), self.rows.cpu(), None if self.wrench is None else self.wrench.cpu())

  def __len__(self):
    return int(self.count.shape[0])

  def tuples(self, i):
    """The contacts of env i as pybullet's `getContactPoints` lists them: 14-field tuples (contactFlag, bodyUniqueIdA,
    bodyUniqueIdB, linkIndexA, linkIndexB, positionOnA, positionOnB, contactNormalOnB, contactDistance, normalForce,
    lateralFriction1, lateralFrictionDir1, lateralFriction2, lateralFrictionDir2).  The body ids are slots, -1 the ground."""
    n = min(int(self.count[i]), self.capacity)
    bodies, rows = self.bodies[i, :n].cpu().tolist(), self.rows[i, :n].cpu().tolist()
    out = []
    for (a, b), r in zip(bodies, rows):
      f = {k: (r[o] if w == 1 else tuple(r[o:o + w])) for k, (o, w) in FIELDS.items()}
      out.append((CONTACT_FLAG, a, b, LINK_INDEX, LINK_INDEX, f['position_on_a'], f['position_on_b'], f['normal_on_b'],
                  f['distance'], f['normal_force'], f['lateral_friction1'], f['lateral_friction_dir1'],
                  f['lateral_friction2'], f['lateral_friction_dir2']))
    return out


def empty(B, capacity, L, wrench, device):
  """Uninitialised tensors for `srl_contact_points` to fill."""
  return ContactPoints(torch.empty(B, dtype=torch.int32, device=device),
                       torch.empty((B, capacity, 2), dtype=torch.int32, device=device),
                       torch.empty((B, capacity, ROW_WORDS), dtype=torch.float32, device=device),
                       torch.empty((B, L, WRENCH_WORDS), dtype=torch.float32, device=device) if wrench else None)


def check_out(out, B, L, wrench, device):
  """`out` as the export needs it: contiguous tensors of the right types and shapes on the env's device; its capacity."""
  C = int(out.rows.shape[1]) if out.rows.dim() == 3 else -1
  want = [(out.count, (B,), torch.int32), (out.bodies, (B, C, 2), torch.int32), (out.rows, (B, C, ROW_WORDS), torch.float32)]
  if wrench:
    if out.wrench is None:
      raise ValueError('out has no wrench tensor')
    want.append((out.wrench, (B, L, WRENCH_WORDS), torch.float32))
  for t, shape, dt in want:
    if tuple(t.shape) != shape or t.dtype != dt or t.device != device or not t.is_contiguous():
      raise ValueError('out must hold contiguous tensors on {}: count int32 [B], bodies int32 [B, C, 2], rows float32 '
                       '[B, C, {}], wrench float32 [B, L, {}]'.format(device, ROW_WORDS, WRENCH_WORDS))
  return C
