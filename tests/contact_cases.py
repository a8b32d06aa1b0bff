"""`srl_contact_points` (include/stackrl_hip.h "Contact points") restated in numpy: a state record, as `get_state` returns it,
decoded into (count, bodies, rows, wrench) in float32 with the kernel's operation order.  The blob's offsets are restated as
`layout()` of csrc/env_host.h builds them, from the `#define`s tests/state_cases.py reads.

A fused multiply-add is evaluated exactly: the product of two float32 is exact in float64, the float64 sum is made with its
rounding error (TwoSum) and rounded to odd where it is inexact, so that the final rounding to float32 is the single rounding
of the fused operation (53 >= 2 * 24 + 2 bits).

`decode(..., variant=...)` also states five WRONG readings of the definition, for tests/test_contact_cases.py to show that
its cases tell them apart."""
import numpy as np

import state_cases
from state_cases import D, blob_words, nslots

F32, F64 = np.float32, np.float64
ROW_WORDS, WRENCH_WORDS = 20, 8
GMAXP, GM_WORDS, MAN_WORDS, MP_WORDS = D['SRL_GMAXP'], D['SRL_GM_WORDS'], D['SRL_MAN_WORDS'], D['SRL_MP_WORDS']
GM_VID, GM_DIST, GM_IN, GM_T1, GM_T2 = (D[k] for k in ('SRL_GM_VID', 'SRL_GM_DIST', 'SRL_GM_IN', 'SRL_GM_T1', 'SRL_GM_T2'))
HDR_PAD = state_cases.pad4(state_cases.HDR_WORDS)
VARIANTS = ('transposed_rotation', 'swapped_bodies', 'impulses_not_divided', 'pairs_first', 'torque_about_origin')


def offsets(L):
  """Word offsets of the blob's parts for episode_length L (csrc/env_host.h `layout`), and NS, NP."""
  NS, NP = nslots(L), max(L * (L - 1) // 2, 1)
  o = {'V': 0}
  o['X'] = 8 * L
  o['Q'] = o['X'] + 4 * L
  o['PX'] = o['Q'] + 4 * L
  o['PQ'] = o['PX'] + 4 * L
  o['MESH'] = o['PQ'] + 4 * L
  o['GM'] = o['MESH'] + L
  o['MAN'] = o['GM'] + GM_WORDS * L
  o['SOP'] = o['MAN'] + MAN_WORDS * NS
  o['POS'] = o['SOP'] + NP
  o['COL'] = o['POS'] + NS
  o['END'] = o['COL'] + NS
  return o, NS, NP


def max_points(L):
  return GMAXP * L + 4 * nslots(L)


def pair_bodies(p):
  """Bodies (i < j) of pair id p = j (j - 1) / 2 + i."""
  j = int((1 + (1 + 8 * p) ** 0.5) / 2)
  while j * (j - 1) // 2 > p:
    j -= 1
  while (j + 1) * j // 2 <= p:
    j += 1
  return p - j * (j - 1) // 2, j


def pair_id(i, j):
  return j * (j - 1) // 2 + i


def fma(a, b, c):
  """float32 fma(a, b, c), exactly (see the module's docstring)."""
  a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
  p, c = a.astype(F64) * b.astype(F64), c.astype(F64)
  s = p + c
  t = s - p
  err = (p - (s - t)) + (c - t)
  even = (s.view(np.int64) & 1) == 0
  odd = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
  return odd.astype(F32)


def rotation(q):
  """`quat_to_mat` of csrc/srl_device.h: q float32 [n, 4] (xyzw) -> R float32 [n, 3, 3]."""
  q = np.asarray(q, F32)
  x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
  xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
  one, two = F32(1), F32(2)
  R = np.stack([one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
                two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
                two * (xz - wy), two * (yz + wx), one - two * (xx + yy)], -1).astype(F32)
  return R.reshape(-1, 3, 3)


def mmul_add(R, a, x):
  """x + R a per row: fma(R_i0, a.x, fma(R_i1, a.y, fma(R_i2, a.z, x_i)))."""
  return np.stack([fma(R[:, i, 0], a[:, 0], fma(R[:, i, 1], a[:, 1], fma(R[:, i, 2], a[:, 2], x[:, i]))) for i in range(3)], -1)


def cross(a, b):
  return np.stack([fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])),
                   fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], -1)


def plane_space(n):
  """`plane_space` of csrc/srl_device.h (Bullet's btPlaneSpace1), n float32 [m, 3] -> (p, q)."""
  n = np.asarray(n, F32).reshape(-1, 3)
  nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
  zero, one = np.zeros_like(nx), F32(1)
  with np.errstate(divide='ignore', invalid='ignore'):
    a1 = ny * ny + nz * nz
    k1 = one / np.sqrt(a1)
    p1 = np.stack([zero, -nz * k1, ny * k1], -1)
    q1 = np.stack([a1 * k1, -nx * p1[:, 2], nx * p1[:, 1]], -1)
    a2 = nx * nx + ny * ny
    k2 = one / np.sqrt(a2)
    p2 = np.stack([-ny * k2, nx * k2, zero], -1)
    q2 = np.stack([-nz * p2[:, 1], nz * p2[:, 0], a2 * k2], -1)
  first = (np.abs(nz) > F32(0.70710678))[:, None]
  return np.where(first, p1, p2).astype(F32), np.where(first, q1, q2).astype(F32)


def com_vertices(pool):
  """Per mesh its vertices in the centre-of-mass frame as `srl_load_meshes` makes them: float32 differences."""
  out = []
  for m in range(len(pool)):
    v, _, mc = pool.mesh(m)
    out.append((np.asarray(v, F32) - np.asarray(mc[1:4], F32)[None]).astype(F32))
  return out


def decode(record, L, dt, verts, last_only=False, capacity=None, with_wrench=True, out=None, variant=None):
  """One env.  record: the int32 words of its state record (or of its header and blob alone); L: episode_length; dt:
  sim_time_step; verts: `com_vertices(pool)`.  Returns (count, bodies int32 [C, 2], rows float32 [C, ROW_WORDS], wrench float32
  [L, 8] or None); `out` = (bodies, rows) arrays to write the first min(count, C) rows into, the rest untouched (default: new
  arrays of zeros)."""
  assert variant is None or variant in VARIANTS
  rec = np.ascontiguousarray(record, np.int32)
  nb = int(rec[0])
  gi = rec[HDR_PAD:HDR_PAD + blob_words(L)]
  gf = gi.view(F32)
  o, NS, NP = offsets(L)
  dt = F32(dt)
  X = gf[o['X']:o['X'] + 4 * L].reshape(L, 4)[:, :3]
  R = rotation(gf[o['Q']:o['Q'] + 4 * L].reshape(L, 4))
  if variant == 'transposed_rotation':
    R = R.transpose(0, 2, 1)
  # ---- the candidates in order: (a, b, position on A, position on B, normal, dist, impulses)
  A, Bb, la, lb, nrm, dist, imp, is_ground = [], [], [], [], [], [], [], []
  for b in range(nb):
    g = o['GM'] + GM_WORDS * b
    mesh = int(gi[o['MESH'] + b])
    for k in range(int(gi[g])):
      A.append(b); Bb.append(-1); is_ground.append(True)
      la.append(verts[mesh][int(gi[g + GM_VID + k])]); lb.append(np.zeros(3, F32)); nrm.append(np.array([0, 0, 1], F32))
      dist.append(gf[g + GM_DIST + k]); imp.append([gf[g + GM_IN + k], gf[g + GM_T1 + k], gf[g + GM_T2 + k]])
  pairs = ([], [], [], [], [], [], [], [])
  for sl in range(NS):
    pid = int(gi[o['POS'] + sl])
    if pid < 0:
      continue
    i, j = pair_bodies(pid)
    m = o['MAN'] + MAN_WORDS * sl
    for k in range(int(gi[m])):
      q = m + 4 + MP_WORDS * k
      for lst, v in zip(pairs, (i, j, gf[q:q + 3], gf[q + 3:q + 6], gf[q + 6:q + 9], gf[q + 9], list(gf[q + 10:q + 13]), False)):
        lst.append(v)
  cols = [A, Bb, la, lb, nrm, dist, imp, is_ground]
  if variant == 'pairs_first':
    cols = [p + c for p, c in zip(pairs, cols)]
  else:
    cols = [c + p for p, c in zip(pairs, cols)]
  A, Bb = np.array(cols[0], np.int64), np.array(cols[1], np.int64)
  n = len(A)
  la, lb, nrm = (np.array(c, F32).reshape(n, 3) for c in cols[2:5])
  dist, imp, gnd = np.array(cols[5], F32), np.array(cols[6], F32).reshape(n, 3), np.array(cols[7], bool)
  # ---- the rows
  rows = np.zeros((n, ROW_WORDS), F32)
  if n:
    pa = mmul_add(R[A], la, X[A])
    jb = np.where(gnd, 0, Bb)
    pb = np.where(gnd[:, None], np.stack([pa[:, 0], pa[:, 1], np.zeros(n, F32)], -1), mmul_add(R[jb], lb, X[jb]))
    t1, t2 = plane_space(nrm)
    force = imp if variant == 'impulses_not_divided' else (imp / dt).astype(F32)
    rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9] = pa, pb, nrm, dist
    rows[:, 10], rows[:, 11], rows[:, 12:15], rows[:, 15], rows[:, 16:19] = force[:, 0], force[:, 1], t1, force[:, 2], t2
  a_out, b_out = A.copy(), Bb.copy()
  if variant == 'swapped_bodies':          # the pair rows the other way round: the normal then points from A towards B
    a_out, b_out = np.where(gnd, A, Bb), np.where(gnd, Bb, A)
    rows[~gnd, 0:3], rows[~gnd, 3:6] = rows[~gnd, 3:6].copy(), rows[~gnd, 0:3].copy()
  # ---- the wrench: every contact, whatever last_only and capacity say
  wrench = None
  if with_wrench:
    wrench = np.zeros((L, WRENCH_WORDS), F32)
    if n:
      F = fma(rows[:, 16:19], rows[:, 15:16], fma(rows[:, 12:15], rows[:, 11:12], rows[:, 6:9] * rows[:, 10:11]))
      for b in range(nb):
        f, t, cnt = np.zeros(3, F32), np.zeros(3, F32), 0
        x = np.zeros((1, 3), F32) if variant == 'torque_about_origin' else X[b:b + 1]
        for r in range(n):
          if a_out[r] == b:
            Fr, p = F[r:r + 1], rows[r:r + 1, 0:3]
          elif b_out[r] == b:
            Fr, p = -F[r:r + 1], rows[r:r + 1, 3:6]
          else:
            continue
          f = f + Fr[0]
          t = t + cross(p - x, Fr)[0]
          cnt += 1
        wrench[b, 0:3], wrench[b, 3], wrench[b, 4:7] = f, F32(cnt), t
  # ---- selection and capacity
  keep = np.ones(n, bool) if not last_only else (a_out == nb - 1) | (b_out == nb - 1)
  sel = np.flatnonzero(keep)
  count = len(sel)
  C = max_points(L) if capacity is None else int(capacity)
  if out is None:
    out = (np.zeros((C, 2), np.int32), np.zeros((C, ROW_WORDS), F32))
  bodies_o, rows_o = out
  w = min(count, C)
  bodies_o[:w, 0], bodies_o[:w, 1] = a_out[sel[:w]], b_out[sel[:w]]
  rows_o[:w] = rows[sel[:w]]
  return count, bodies_o, rows_o, wrench


# ------------------------------------------------------------------------------------------------ synthetic records
def empty_record(L):
  """Header and blob of an env with no body: every manifold slot free."""
  rec = np.zeros(HDR_PAD + blob_words(L), np.int32)
  o, NS, NP = offsets(L)
  b = rec[HDR_PAD:]
  b[o['SOP']:o['SOP'] + NP] = -1
  b[o['POS']:o['POS'] + NS] = -1
  b.view(F32)[o['Q']:o['Q'] + 4 * L].reshape(L, 4)[:, 3] = 1.0
  return rec


def put_body(rec, L, b, x, q, mesh):
  o, _, _ = offsets(L)
  gi = rec[HDR_PAD:]
  gf = gi.view(F32)
  gf[o['X'] + 4 * b:o['X'] + 4 * b + 3] = np.asarray(x, F32)
  gf[o['Q'] + 4 * b:o['Q'] + 4 * b + 4] = np.asarray(q, F32)
  gi[o['MESH'] + b] = mesh
  rec[0] = max(int(rec[0]), b + 1)


def put_ground(rec, L, b, points):
  """points: [(vid, dist, in, it1, it2)], at most 4."""
  o, _, _ = offsets(L)
  gi = rec[HDR_PAD:]
  gf = gi.view(F32)
  g = o['GM'] + GM_WORDS * b
  gi[g] = len(points)
  for k, (vid, dist, i0, i1, i2) in enumerate(points):
    gi[g + GM_VID + k] = vid
    gf[g + GM_DIST + k], gf[g + GM_IN + k], gf[g + GM_T1 + k], gf[g + GM_T2 + k] = dist, i0, i1, i2


def put_pair(rec, L, sl, i, j, points):
  """points: [(la3, lb3, n3, dist, in, it1, it2)], at most 4, in manifold slot sl for the bodies i < j."""
  o, _, _ = offsets(L)
  gi = rec[HDR_PAD:]
  gf = gi.view(F32)
  pid = pair_id(i, j)
  gi[o['POS'] + sl], gi[o['SOP'] + pid] = pid, sl
  m = o['MAN'] + MAN_WORDS * sl
  gi[m] = len(points)
  for k, (la, lb, n, dist, i0, i1, i2) in enumerate(points):
    q = m + 4 + MP_WORDS * k
    gf[q:q + 3], gf[q + 3:q + 6], gf[q + 6:q + 9] = np.asarray(la, F32), np.asarray(lb, F32), np.asarray(n, F32)
    gf[q + 9], gf[q + 10], gf[q + 11], gf[q + 12] = dist, i0, i1, i2
