"""The push test's three hooks (include/stackrl_hip.h "Push test") restated in numpy, one env at a time, in float32 with the
kernels' operation order: `kick` (the selection, the two layouts, the untouched slots) and `rows_summary` (the rows perr oerr
dz speed and the eight summary words, their slot order and NaN rule), with the acos polynomial of csrc/srl_device.h.  The
fused dot product is evaluated exactly (contact_cases.fma).

Layouts are those of `srl_get_state` / `srl_get_velocities` with L slots: poses [L, 8] = x y z qx qy qz qw id, velocities
[L, 8] = v xyz, -, w xyz, -.  `variant=...` states WRONG readings of the definition, for tests/test_push_cases.py to show that
its cases tell them apart."""
import numpy as np

from contact_cases import HDR_PAD, fma, offsets
from state_cases import blob_words

F32 = np.float32
ROW_WORDS, SUMMARY_WORDS = 4, 8
KICK_ALL, KICK_LAST = -1, -2
VARIANTS = ('no_fabs', 'slots_le_nb', 'last_hits_nb', 'sum_reversed', 'nan_not_moved', 'ref_nb_ignored')
_PI = F32(3.14159265358979)
_ACOS = [F32(c) for c in (-0.0012624911, 0.0066700901, -0.0170881256, 0.0308918810, -0.0501743046, 0.0889789874, -0.2145988016,
                          1.5707963050)]


def acos(x):
  """`srl_acosf` of csrc/srl_device.h (A&S 4.4.46), float32, one rounding per operation."""
  x = F32(x)
  a = np.abs(x)
  if a > F32(1):
    a = F32(1)
  p = _ACOS[0]
  for c in _ACOS[1:]:
    p = F32(F32(p * a) + c)
  r = F32(np.sqrt(F32(F32(1) - a)) * p)
  return F32(_PI - r) if x < F32(0) else r


def dot(a, b):
  """fma(a.x, b.x, fma(a.y, b.y, a.z * b.z))."""
  return F32(fma(a[0], b[0], fma(a[1], b[1], F32(a[2]) * F32(b[2]))))


def clamp_nb(nb, L):
  return min(max(int(nb), 0), L)


def distance(ref7, now7, variant=None):
  """(perr, oerr) of a body at `now7` from the reference pose `ref7` (x y z qx qy qz qw): the reward's `body_discount`."""
  ref7, now7 = np.asarray(ref7, F32), np.asarray(now7, F32)
  with np.errstate(invalid='ignore'):
    d = (ref7[:3] - now7[:3]).astype(F32)
    perr = F32(np.sqrt(dot(d, d)))
    a, q = ref7[3:7], now7[3:7]
    dw = F32(F32(F32(a[0] * q[0]) + F32(a[1] * q[1])) + F32(F32(a[2] * q[2]) + F32(a[3] * q[3])))
    if variant != 'no_fabs':
      dw = np.abs(dw)
    oerr = F32(F32(2) * acos(np.fmin(dw, F32(1))))
  return perr, oerr


def kick(vel, nb, dv, per_body, select, variant=None):
  """The velocities [L, 8] of one env after `srl_kick`: dv is [L, 8] (per_body) or [8]; select KICK_ALL, KICK_LAST or a slot."""
  vel = np.array(vel, F32)
  L = vel.shape[0]
  dv = np.asarray(dv, F32)
  assert dv.shape == ((L, 8) if per_body else (8,))
  nb = clamp_nb(nb, L)
  top = nb + 1 if variant == 'slots_le_nb' else nb
  for b in range(min(top, L)):
    target = b if select == KICK_ALL else ((nb if variant == 'last_hits_nb' else nb - 1) if select == KICK_LAST else select)
    if b != target:
      continue
    d = dv[b] if per_body else dv
    for k in (0, 1, 2, 4, 5, 6):
      vel[b, k] = F32(vel[b, k] + d[k])
  return vel


def rows_summary(poses, vel, nb, place, ref=None, ref_nb=None, tol=(0.0, 0.0), variant=None):
  """(rows float32 [L, 4], summary float32 [8]) of one env: poses, vel [L, 8]; place [L, 7+] the place poses; ref [L, 8] or
  None with its body count ref_nb (None: every row counts)."""
  poses, vel, place = np.asarray(poses, F32), np.asarray(vel, F32), np.asarray(place, F32)
  L = poses.shape[0]
  nb = clamp_nb(nb, L)
  tp, to = F32(tol[0]), F32(tol[1])
  rows = np.zeros((L, ROW_WORDS), F32)
  spin = np.zeros(L, F32)
  top = min(nb + 1, L) if variant == 'slots_le_nb' else nb
  for b in range(top):
    from_ref = ref is not None and (ref_nb is None or variant == 'ref_nb_ignored' or b < int(ref_nb))
    r = np.asarray(ref, F32)[b] if from_ref else place[b]
    perr, oerr = distance(r[:7], poses[b, :7], variant)
    with np.errstate(invalid='ignore'):
      rows[b] = (perr, oerr, F32(poses[b, 2] - r[2]), F32(np.sqrt(dot(vel[b, 0:3], vel[b, 0:3]))))
      spin[b] = F32(np.sqrt(dot(vel[b, 4:7], vel[b, 4:7])))
  moved, mp, mo, sp, mdz, mv, mw = F32(0), F32(0), F32(0), F32(0), F32(0), F32(0), F32(0)
  order = range(top - 1, -1, -1) if variant == 'sum_reversed' else range(top)
  with np.errstate(invalid='ignore'):
    for b in order:
      p, o = rows[b, 0], rows[b, 1]
      beyond = (p > tp or o > to) if variant == 'nan_not_moved' else not (p <= tp and o <= to)
      if beyond:
        moved = F32(moved + F32(1))
      mp, mo = np.fmax(mp, p), np.fmax(mo, o)
      sp = F32(sp + p)
      mdz = np.fmin(mdz, rows[b, 2])
      mv, mw = np.fmax(mv, rows[b, 3]), np.fmax(mw, spin[b])
  return rows, np.array([F32(nb), moved, mp, mo, sp, mdz, mv, mw], F32)


def place_poses(record, L):
  """[L, 7] place poses (x y z qx qy qz qw) of one env's state record (or of its header and blob alone)."""
  gf = np.asarray(record, np.int32)[HDR_PAD:HDR_PAD + blob_words(L)].view(F32)
  o = offsets(L)[0]
  px = gf[o['PX']:o['PX'] + 4 * L].reshape(L, 4)
  pq = gf[o['PQ']:o['PQ'] + 4 * L].reshape(L, 4)
  return np.concatenate([px[:, :3], pq], axis=1).astype(F32)


def same_bits(a, b):
  """Equal bit for bit, a NaN on both sides counting as equal: IEEE 754 leaves a NaN's sign and payload to the implementation."""
  a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
  return a.shape == b.shape and bool(np.all((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))
