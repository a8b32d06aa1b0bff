"""CPU tests of the contact-point definition (include/stackrl_hip.h "Contact points") as tests/contact_cases.py restates it, on
synthetic state records: the blob offsets, the tangent rule, two hand-built piles held to values worked out by hand, the empty
world, and five wrong readings of the definition that the piles must tell apart.  tests/test_contacts_gpu.py holds the kernel
to the same restatement bit for bit."""
import numpy as np
import pytest

import contact_cases as cc
import state_cases as sc

F32, F64 = np.float32, np.float64
DT = 1.0 / 64            # dyadic, like every number of the piles: the hand-made values are exact in float32
L = 8
# a mesh of four vertices in its centre-of-mass frame
VERTS = [np.array([[0.25, 0, -0.125], [-0.25, 0.25, -0.125], [-0.25, -0.25, -0.125], [0, 0, 0.25]], F32),
         np.array([[0.5, 0.125, -0.25], [-0.125, 0.25, 0.0625], [0.0625, -0.5, 0.125], [0.25, 0.5, 0.375]], F32)]


@pytest.mark.parametrize('L', [1, 8, 9, 32])
def test_offsets_add_up_to_the_blob(L):
  o, NS, NP = cc.offsets(L)
  assert sc.pad4(o['END']) == sc.blob_words(L) and NS == sc.nslots(L)
  order = ['V', 'X', 'Q', 'PX', 'PQ', 'MESH', 'GM', 'MAN', 'SOP', 'POS', 'COL', 'END']
  assert all(o[a] <= o[b] for a, b in zip(order, order[1:])) and o['V'] == 0
  assert cc.max_points(L) == 4 * L + 4 * NS


def test_fma_is_the_single_rounding():
  # a b = 2^-24 (1 - 2^-46): 1 + 2^-23 + a b lies just below the tie between 1 + 2^-23 and 1 + 2^-22.  The float64 sum is the
  # tie itself, and rounded again it goes to the even neighbour, 1 + 2^-22; the fused operation gives 1 + 2^-23
  a, b, c = F32(2.0 ** -12 * (1 + 2.0 ** -23)), F32(2.0 ** -12 * (1 - 2.0 ** -23)), F32(1 + 2.0 ** -23)
  assert F32(F64(a) * F64(b) + F64(c)) == F32(1 + 2.0 ** -22)
  assert cc.fma(a, b, c) == F32(1 + 2.0 ** -23)
  assert cc.fma(a, -b, -c) == -F32(1 + 2.0 ** -23)
  assert cc.fma(F32(3), F32(5), F32(-7)) == F32(8)


def _bt_plane_space(n):
  """btPlaneSpace1 in float64."""
  x, y, z = (float(c) for c in n)
  if abs(z) > 0.7071067811865476:
    a = y * y + z * z
    k = 1 / np.sqrt(a)
    p = (0.0, -z * k, y * k)
    return p, (a * k, -x * p[2], x * p[1])
  a = x * x + y * y
  k = 1 / np.sqrt(a)
  p = (-y * k, x * k, 0.0)
  return p, (-z * p[1], z * p[0], a * k)


def test_tangents_are_bullets_plane_space_on_both_branches():
  above, below = 0.7072, 0.7070
  normals = [(0, 0, 1), (1, 0, 0), (np.sqrt(1 - above ** 2) * 0.6, np.sqrt(1 - above ** 2) * 0.8, above),
             (np.sqrt(1 - below ** 2) * 0.6, -np.sqrt(1 - below ** 2) * 0.8, -below)]
  n = np.array(normals, F32)
  assert [abs(float(v[2])) > 0.70710678 for v in n] == [True, False, True, False]
  p, q = cc.plane_space(n)
  assert p.dtype == F32 and q.dtype == F32
  for k in range(len(n)):
    ep, eq = _bt_plane_space(n[k])
    np.testing.assert_allclose(p[k], ep, rtol=0, atol=2e-7)
    np.testing.assert_allclose(q[k], eq, rtol=0, atol=2e-7)
    n64 = n[k].astype(F64)
    assert abs(np.dot(p[k], n64)) < 3e-7 and np.allclose(np.cross(n64, p[k]), q[k], rtol=0, atol=3e-7)
  assert p[0].tolist() == [0, -1, 0] and q[0].tolist() == [1, 0, 0]          # solver.h: the ground rows' -y and +x
  assert p[1].tolist() == [0, 1, 0] and q[1].tolist() == [0, 0, 1]


# ------------------------------------------------------------------------------------------------ the piles
G0 = [(2, -2.0 ** -10, 0.5, 0.125, -0.25), (0, 2.0 ** -9, 0.25, -0.0625, 0.03125), (1, -2.0 ** -8, 1.0, 0.5, 0.75)]


def pile_ground():
  """One body on the ground with three points."""
  rec = cc.empty_record(L)
  cc.put_body(rec, L, 0, (1, 2, 0.125), (0, 0, 0, 1), 0)
  cc.put_ground(rec, L, 0, G0)
  return rec


def expected_ground():
  x = np.array([1, 2, 0.125])
  rows, F, arm = [], [], []
  for vid, dist, i0, i1, i2 in G0:
    pa = x + VERTS[0][vid].astype(F64)
    fn, f1, f2 = i0 * 64, i1 * 64, i2 * 64
    rows.append(list(pa) + [pa[0], pa[1], 0] + [0, 0, 1, dist, fn, f1, 0, -1, 0, f2, 1, 0, 0, 0])
    F.append((f2, -f1, fn))                                 # fn (0, 0, 1) + f1 (0, -1, 0) + f2 (1, 0, 0)
    arm.append(pa - x)
  wrench = np.zeros((L, 8))
  wrench[0, 0:3], wrench[0, 3], wrench[0, 4:7] = np.sum(F, 0), 3, np.sum(np.cross(arm, F), 0)
  return np.array([[0, -1]] * 3), np.array(rows, F64), wrench


X0, X1 = np.array([0, 0, 0.25]), np.array([0.125, 0.0625, 0.75])
GP = [(0, -2.0 ** -10, 2.0, 0.25, -0.5), (2, -2.0 ** -11, 1.5, -0.125, 0.0625)]
# la, lb, n (from body 1, on top, down to body 0), dist, impulses
PP = [((0.25, 0.125, 0.25), (-0.25, 0.125, 0.0625), (0, 0, -1), -2.0 ** -9, 1.0, 0.25, -0.125),
      ((-0.25, 0.125, 0.25), (-0.25, -0.375, 0.0625), (0, 0, -1), -2.0 ** -10, 0.5, -0.5, 0.375),
      ((0.125, -0.25, 0.25), (-0.25, 0.0625, -0.3125), (0, 0, -1), 2.0 ** -12, 0.0, 0.0, 0.0),
      ((0.0625, 0.03125, 0.25), (-0.25, -0.0625, -0.03125), (0, 0, -1), -2.0 ** -8, 0.75, 0.0625, 0.03125)]
PAIR_SLOT = 3


def pile_pair():
  """Two bodies, the lower one on the ground with two points, one pair manifold of four points in slot 3; body 1 is turned 90
  degrees about x, then 90 degrees about z: q = (1/2, 1/2, 1/2, 1/2), R (a, b, c) = (c, a, b)."""
  rec = cc.empty_record(L)
  cc.put_body(rec, L, 0, X0, (0, 0, 0, 1), 0)
  cc.put_body(rec, L, 1, X1, (0.5, 0.5, 0.5, 0.5), 1)
  cc.put_ground(rec, L, 0, GP)
  cc.put_pair(rec, L, PAIR_SLOT, 0, 1, PP)
  return rec


def expected_pair():
  bodies, rows, F0, arm0, F1, arm1 = [], [], [], [], [], []
  for vid, dist, i0, i1, i2 in GP:
    pa = X0 + VERTS[0][vid].astype(F64)
    fn, f1, f2 = i0 * 64, i1 * 64, i2 * 64
    bodies.append((0, -1))
    rows.append(list(pa) + [pa[0], pa[1], 0] + [0, 0, 1, dist, fn, f1, 0, -1, 0, f2, 1, 0, 0, 0])
    F0.append((f2, -f1, fn)); arm0.append(pa - X0)
  for la, lb, n, dist, i0, i1, i2 in PP:
    pa = X0 + np.array(la)
    rb = np.array([lb[2], lb[0], lb[1]])                    # Rz(90) Rx(90) (a, b, c) = (c, a, b)
    pb = X1 + rb
    fn, f1, f2 = i0 * 64, i1 * 64, i2 * 64
    bodies.append((0, 1))                                   # n points from body 1 to body 0: A = 0, B = 1
    rows.append(list(pa) + list(pb) + [0, 0, -1, dist, fn, f1, 0, 1, 0, f2, 1, 0, 0, 0])     # btPlaneSpace1 of -z: +y, +x
    F = np.array([f2, f1, -fn])
    F0.append(F); arm0.append(pa - X0)
    F1.append(-F); arm1.append(rb)
  wrench = np.zeros((L, 8))
  wrench[0, 0:3], wrench[0, 3], wrench[0, 4:7] = np.sum(F0, 0), 6, np.sum(np.cross(arm0, F0), 0)
  wrench[1, 0:3], wrench[1, 3], wrench[1, 4:7] = np.sum(F1, 0), 4, np.sum(np.cross(arm1, F1), 0)
  return np.array(bodies), np.array(rows, F64), wrench


PILES = {'ground': (pile_ground, expected_ground), 'pair': (pile_pair, expected_pair)}


@pytest.mark.parametrize('name', sorted(PILES))
def test_pile_equals_the_values_made_by_hand(name):
  rec, (bodies, rows, wrench) = PILES[name][0](), PILES[name][1]()
  n = len(rows)
  count, b, r, w = cc.decode(rec, L, DT, VERTS)
  assert count == n and b.shape == (cc.max_points(L), 2) and r.dtype == F32
  assert np.array_equal(b[:n], bodies) and np.array_equal(r[:n].astype(F64), rows)
  assert not b[n:].any() and not r[n:].any()
  assert np.array_equal(w.astype(F64), wrench)
  # `last_only`: the rows of the last placed body, in their order
  keep = [k for k in range(n) if (rec[0] - 1) in bodies[k]]
  count, b, r, w = cc.decode(rec, L, DT, VERTS, last_only=True)
  assert count == len(keep) and np.array_equal(b[:count], bodies[keep]) and np.array_equal(r[:count].astype(F64), rows[keep])
  assert np.array_equal(w.astype(F64), wrench)            # the wrench covers every contact all the same
  if name == 'pair':
    assert keep == [2, 3, 4, 5]
  # capacity: the true count, the first rows, the rest untouched
  for C in (n - 1, n, 1):
    out = (np.full((C + 2, 2), 77, np.int32), np.full((C + 2, cc.ROW_WORDS), 7.5, F32))
    count, b, r, w = cc.decode(rec, L, DT, VERTS, capacity=C, out=(out[0][:C], out[1][:C]))
    m = min(n, C)
    assert count == n and np.array_equal(out[0][:m], bodies[:m]) and np.array_equal(out[1][:m].astype(F64), rows[:m])
    assert (out[0][m:] == 77).all() and (out[1][m:] == 7.5).all()
    assert np.array_equal(w.astype(F64), wrench)


def test_empty_world_has_no_contact_and_writes_nothing():
  rec = cc.empty_record(L)
  out = (np.full((5, 2), 77, np.int32), np.full((5, cc.ROW_WORDS), 7.5, F32))
  count, b, r, w = cc.decode(rec, L, DT, VERTS, capacity=5, out=out)
  assert count == 0 and (b == 77).all() and (r == 7.5).all() and not w.any()
  rec[0] = 2                                                # two bodies in the air: still nothing
  count, b, r, w = cc.decode(rec, L, DT, VERTS, capacity=5, out=out)
  assert count == 0 and (b == 77).all() and (r == 7.5).all() and not w.any()


@pytest.mark.parametrize('variant', cc.VARIANTS)
def test_the_piles_tell_a_wrong_reading_apart(variant):
  """transposed rotation; bodies the other way round than the normal's sign demands (the kernel's n points from j to i, so A = i
  unswapped is right and the swap is the wrong reading); impulses not divided by dt; pair points before ground points; torque
  about the origin."""
  differs = []
  for name in sorted(PILES):
    rec = PILES[name][0]()
    right, wrong = cc.decode(rec, L, DT, VERTS), cc.decode(rec, L, DT, VERTS, variant=variant)
    differs.append(right[0] != wrong[0] or any(not np.array_equal(a, b) for a, b in zip(right[1:], wrong[1:])))
  assert any(differs), variant
  if variant in ('transposed_rotation', 'swapped_bodies', 'pairs_first'):
    assert differs == [False, True]                         # (only the pile with a rotated body and a pair can tell)
