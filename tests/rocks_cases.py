"""The rock generator's definition (include/stackrl_rocks.h) restated in numpy: float64 predicates on float32 points, the
Philox stream, `scipy.special.ndtri`.  Stage by stage what csrc/rocks.hip computes, with the same loop bounds; the wrong
variants (`predicate`, `halving`, `sort_axes`) exist so that tests/test_rocks_cases.py can show its checks tell them apart.
No GPU needed."""
import numpy as np
from scipy import special

from stackrl_amd import assets

MAX_VERTS, MAX_TRIS, MAX_POINTS = 128, 252, 386
QCAP = 3 * MAX_TRIS + 4
TAG = 0x524f434b
DENSITY_DRAW = 0xffffffff
OK, OVERFLOW, DEGENERATE = 0, 1, 2
POINTS = (8, 26, 98, 386)
DEFAULTS = dict(radius=0.0625, irregularity=0.5, extents=(1., 1 / 2, 1 / 3), subdivisions=3, density=(2200., 2600.), fit=0, seed=11)


# ------------------------------------------------------------------------------------------------ stage 1: points
def philox4x32_10(counter, key):
  """Philox4x32-10: counter uint [..., 4], key uint [..., 2] -> uint64 [..., 4] (32-bit words)."""
  c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
  k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
  m = np.uint64(0xffffffff)
  for _ in range(10):
    p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
    c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m]
    k = [(k[0] + np.uint64(0x9E3779B9)) & m, (k[1] + np.uint64(0xBB67AE85)) & m]
  return np.stack(c, axis=-1)


def draws(index, numbers, seed):
  """The uniform numbers u = (x + 0.5) 2^-32 of rock `index` for the draw `numbers` (word 0 of one Philox call each)."""
  numbers = np.asarray(numbers, dtype=np.uint64)
  index = int(index) % 2 ** 64
  counter = np.zeros(numbers.shape + (4,), dtype=np.uint64)
  counter[..., 0], counter[..., 1], counter[..., 2] = index & 0xffffffff, index >> 32, numbers
  x = philox4x32_10(counter, np.array([int(seed) % 2 ** 32, TAG], dtype=np.uint64))[..., 0]
  return (x.astype(np.float64) + 0.5) * 2.0 ** -32


def parent_table():
  """[386, 2]: the two points a point is the midpoint of (rows 0..7: -1), read off `assets._subdivide` on the box."""
  v = np.zeros((8, 3))
  t = assets._BOX_TRIS.copy()
  par = -np.ones((MAX_POINTS, 2), dtype=np.int64)
  for _ in range(3):
    nv = len(v)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    ue = np.unique(e, axis=0)
    v, t = assets._subdivide(v, t)
    par[nv:len(v)] = ue
  assert len(v) == MAX_POINTS
  return par


_PARENTS = parent_table()


def truncated_normal(u, irregularity):
  """u in (0, 1) -> the truncated standard normal on [-1 / irregularity, 1 / irregularity] by the inverse CDF, float64."""
  bound = 1.0 / irregularity
  Fa = special.ndtr(-bound)
  return np.clip(special.ndtri(Fa + u * ((1.0 - Fa) - Fa)), -bound, bound)


def noise(index, radius=0.0625, irregularity=0.5, subdivisions=3, seed=11, halving=True, **_):
  """float64 [P, 3]: the noise of every point (scale_l * the truncated normal of draw 3 k + j), and its scale [P]."""
  P = POINTS[subdivisions]
  irr, radius = float(np.float32(irregularity)), float(np.float32(radius))
  level = np.searchsorted(np.array(POINTS), np.arange(P), side='right')       # 0 for k < 8, 1 for k < 26, ...
  scale = irr * radius * (0.5 ** level if halving else np.ones(P))
  x = truncated_normal(draws(index, np.arange(3 * P).reshape(P, 3), seed), irr)
  return scale[:, None] * x, scale


def points(index, radius=0.0625, irregularity=0.5, extents=(1., 1 / 2, 1 / 3), subdivisions=3, seed=11, halving=True, **_):
  """Stage 1: float32 [P, 3]."""
  P = POINTS[subdivisions]
  r = float(np.float32(radius))
  e = np.array([float(np.float32(x)) for x in extents])
  half = e * 2.0 * r / np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) / 2.0
  nz, _ = noise(index, radius, irregularity, subdivisions, seed, halving)
  pd = np.zeros((P, 3))
  k = np.arange(8)
  sign = np.stack([(k >> 2) & 1, (k >> 1) & 1, k & 1], axis=1) * 2.0 - 1.0
  pd[:8] = sign * half + nz[:8]
  start, end = 8, 26
  while start < P:
    pa, pb = _PARENTS[start:end, 0], _PARENTS[start:end, 1]
    pd[start:end] = (pd[pa] + pd[pb]) / 2.0 + nz[start:end]
    start, end = end, 4 * end - 6
  return pd.astype(np.float32)


def density(index, seed=11, density=(2200., 2600.), **_):
  lo, hi = float(np.float32(density[0])), float(np.float32(density[1]))
  return lo + float(draws(index, DENSITY_DRAW, seed)) * (hi - lo)


# ------------------------------------------------------------------------------------------------ stage 2: hull
def _cross(u, v):
  return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                   u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _dot(u, v):
  return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def pivot(p, a, b, A, B):
  """The point c (not a, not b, not on the line A -> B) with orient(A, B, c, q) <= 0 for every other q, the lowest index among
  equals; -1 without a candidate.  `p` in the predicate's type."""
  e = B - A
  w = p - A
  cr = _cross(e, w)
  cand = np.any(cr != 0, axis=1)
  cand[a] = False
  if b >= 0:
    cand[b] = False
  idx = np.nonzero(cand)[0]
  if len(idx) == 0:
    return -1
  best = idx[0]
  for _ in range(len(p) + 1):                  # a strict total order on non-degenerate input: any order of comparisons ends at its maximum
    d = _dot(cr[best], w[idx])
    beats = (d > 0) | ((d == 0) & (idx < best))
    if not beats.any():
      break
    best = idx[beats][np.argmax(d[beats])]
  return int(best)


def hull(pts, predicate=np.float64):
  """Stage 2 on float32 points [P, 3]: (status, vert_src [nv] ascending, tris [nt, 3] in final numbers, wrap order)."""
  pts = np.asarray(pts, dtype=np.float32)
  p = pts.astype(predicate)
  P = len(p)
  order = np.lexsort((np.arange(P), pts[:, 2], pts[:, 1], pts[:, 0]))
  p0 = int(order[0])
  empty = (np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64))
  p1 = pivot(p, p0, -1, p[p0], p[p0] + np.array([0, 1, 0], dtype=predicate))
  if p1 < 0:
    return (DEGENERATE,) + empty
  lid, src, done, tris = {p0: 0, p1: 1}, [p0, p1], set(), []
  queue, head = [(0, 1)], 0
  while head < len(queue):
    la, lb = queue[head]
    head += 1
    if (la, lb) in done:
      continue
    a, b = src[la], src[lb]
    c = pivot(p, a, b, p[a], p[b])
    if c < 0:
      return (DEGENERATE,) + empty
    if c not in lid:
      if len(src) >= MAX_VERTS:
        return (OVERFLOW,) + empty
      lid[c] = len(src)
      src.append(c)
    lc = lid[c]
    if len(tris) >= MAX_TRIS:
      return (OVERFLOW,) + empty
    edges = [(la, lb), (lb, lc), (lc, la)]
    twice = any(e in done for e in edges) or len(set(edges)) < 3
    done.update(edges)
    if twice:
      return (DEGENERATE,) + empty
    tris.append((la, lb, lc))
    for s, t in edges:
      if (t, s) not in done and len(queue) < QCAP:
        queue.append((t, s))
  nv, nt = len(src), len(tris)
  if any((t, s) not in done for s, t in done) or nv < 4 or nt != 2 * nv - 4:
    return (DEGENERATE,) + empty
  src = np.array(src)
  ta, tb, tc = (p[src[np.array(tris)[:, k]]] for k in range(3))          # convex: every point on or behind every face
  n = _cross(tb - ta, tc - ta)
  w = p[None, :, :] - ta[:, None, :]
  front = (n[:, None, 0] * w[..., 0] + n[:, None, 1] * w[..., 1]) + n[:, None, 2] * w[..., 2] > 0
  front[np.arange(len(tris))[:, None], src[np.array(tris)]] = False      # (a face's own vertices are on it)
  if front.any():
    return (DEGENERATE,) + empty
  rank = np.argsort(np.argsort(src))
  return OK, np.sort(src), rank[np.array(tris)]


# ------------------------------------------------------------------------------------------------ stages 3-5
def mass_inertia(v, t, rho=1.0):
  """Volume, centre of mass and inertia (ixx ixy ixz iyy iyz izz about the centre of mass, density applied) of a closed
  mesh by signed tetrahedra from the origin, float64."""
  v = np.asarray(v, dtype=np.float64)
  a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
  d = _dot(a, _cross(b, c))
  volume = d.sum() / 6.0
  com = ((a + b + c) * d[:, None]).sum(0) / (4.0 * d.sum())
  s = a + b + c
  M = (np.einsum('ni,nj->nij', a, a) + np.einsum('ni,nj->nij', b, b) + np.einsum('ni,nj->nij', c, c) +
       np.einsum('ni,nj->nij', s, s))
  C = (M * d[:, None, None]).sum(0) / 120.0 - volume * np.outer(com, com)
  I = rho * (np.trace(C) * np.eye(3) - C)
  return volume, com, np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]])


def oriented_box(u, t, sort_axes=True):
  """Stage 4 on the hull vertices u (float64, about the centre of mass): the minimum-volume box over (face normal, edge
  projected into the face's plane) pairs.  Returns (R, centre, extents, volume): rows of R the final axes (after the sort,
  the sign fix and the turn about Y), final extents x >= y >= z."""
  nt = len(t)
  k = np.arange(3 * nt)
  es, et = t[k // 3, k % 3], t[k // 3, (k % 3 + 1) % 3]
  keep = es < et
  es, et = es[keep], et[keep]
  best = (np.inf, None)
  for f in range(nt):
    a, b, c = u[t[f, 0]], u[t[f, 1]], u[t[f, 2]]
    n = _cross(b - a, c - a)
    n = n / np.sqrt(_dot(n, n))
    x = _cross(n, np.array([1., 0, 0]) if abs(n[0]) < 0.9 else np.array([0, 1., 0]))
    x = x / np.sqrt(_dot(x, x))
    y = _cross(n, x)
    px, py, h = _dot(u, x), _dot(u, y), _dot(u, n)
    dx, dy = px[et] - px[es], py[et] - py[es]
    ln = np.sqrt(dx * dx + dy * dy)
    ok = ln > 0
    cs, sn = dx[ok] / ln[ok], dy[ok] / ln[ok]
    X = px[None] * cs[:, None] + py[None] * sn[:, None]
    Y = py[None] * cs[:, None] - px[None] * sn[:, None]
    vol = ((X.max(1) - X.min(1)) * (Y.max(1) - Y.min(1))) * (h.max() - h.min())
    j = int(np.argmin(vol))
    if vol[j] < best[0]:
      best = (vol[j], np.stack([cs[j] * x + sn[j] * y, cs[j] * y - sn[j] * x, n]))
  rows = best[1]
  pr = u @ rows.T
  lo, hi = pr.min(0), pr.max(0)
  order = np.argsort(hi - lo, kind='stable') if sort_axes else np.arange(3)
  rows, lo, hi = rows[order], lo[order], hi[order]
  if _dot(rows[0], _cross(rows[1], rows[2])) < 0:
    rows[2], lo[2], hi[2] = -rows[2], -hi[2], -lo[2]
  centre = rows.T @ ((lo + hi) / 2.0)
  ext = hi - lo
  R = np.stack([rows[2], rows[1], -rows[0]])
  return R, centre, ext[::-1].copy(), best[0]


def rock(index=0, pts=None, predicate=np.float64, halving=True, sort_axes=True, **params):
  """One rock by the definition: a dict of status, points, vert_src, tris, verts (float32), xform (float32 [13]), mass_com,
  inertia, metrics and the box volume of stage 4 (before the scale).  `pts`: float32 [P, 3] in place of stage 1."""
  q = dict(DEFAULTS)
  q.update(params)
  pts = points(index, halving=halving, **q) if pts is None else np.asarray(pts, dtype=np.float32)
  status, src, tris = hull(pts, predicate)
  out = {'status': status, 'points': pts, 'vert_src': src, 'tris': tris}
  if status != OK:
    return out
  radius = float(np.float32(q['radius']))
  hp = pts[src].astype(np.float64)
  _, com, _ = mass_inertia(hp, tris)
  u = hp - com
  R, centre, ext, box_volume = oriented_box(u, tris, sort_axes)
  s = radius / np.sqrt(_dot(u, u).max()) if q['fit'] == 0 else 2.0 * radius / ext.max()
  s = s if s < 1.0 else 1.0
  xform = np.concatenate([[s], R.ravel(), com + centre]).astype(np.float32)
  verts = apply_xform(xform, hp).astype(np.float32)
  rho = density(index, q['seed'], q['density'])
  volume, c, inertia = mass_inertia(verts, tris, rho)
  fe = verts.astype(np.float64).max(0) - verts.astype(np.float64).min(0)
  out.update(verts=verts, xform=xform, mass_com=np.concatenate([[rho * volume], c]).astype(np.float32), inertia=inertia.astype(np.float32),
             metrics=np.array([volume, volume / fe.prod(), fe.max() / fe.min(), fe.prod()], dtype=np.float32), box_volume=box_volume,
             scale=s, density=rho)
  return out


def apply_xform(xform, p):
  """final = s R (p - c) in float64, from the float32 values of `xform` [13]."""
  x = np.asarray(xform, dtype=np.float64)
  return x[0] * ((np.asarray(p, dtype=np.float64) - x[10:13]) @ x[1:10].reshape(3, 3).T)


# ------------------------------------------------------------------------------------------------ mesh checks and edge cases
def closed_outward(v, t):
  """A closed two-manifold (every directed edge once, its opposite present, Euler) whose signed volume is positive."""
  e = [(int(a), int(b)) for tri in t for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))]
  s = set(e)
  return (len(s) == len(e) and all((b, a) in s for a, b in s) and len(t) == 2 * len(v) - 4 and
          mass_inertia(v, t)[0] > 0)


def max_outside(v, t, p):
  """The largest signed distance of the points p in front of a face plane of the mesh (<= 0: all behind every face)."""
  v = np.asarray(v, dtype=np.float64)
  a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
  n = _cross(b - a, c - a)
  n = n / np.sqrt(_dot(n, n))[:, None]
  return float((np.asarray(p, dtype=np.float64) @ n.T - _dot(n, a)[None]).max())


def sphere_points(n=200, radius=0.0625):
  """n points on a sphere (a Fibonacci lattice): every one is a hull vertex."""
  k = np.arange(n) + 0.5
  phi, z = np.pi * (1 + 5 ** 0.5) * k, 1 - 2 * k / n
  r = np.sqrt(1 - z * z)
  return (radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)).astype(np.float32)


def coplanar_box(subdivisions=2):
  """The subdivided box without noise: exactly coplanar points on every face (extents are powers of two: midpoints are exact)."""
  P = POINTS[subdivisions]
  k = np.arange(8)
  pd = np.zeros((P, 3))
  pd[:8] = (np.stack([(k >> 2) & 1, (k >> 1) & 1, k & 1], axis=1) * 2.0 - 1.0) * np.array([0.0625, 0.03125, 0.015625])
  pd[8:] = 0
  for i in range(8, P):
    pd[i] = (pd[_PARENTS[i, 0]] + pd[_PARENTS[i, 1]]) / 2.0
  return pd.astype(np.float32)


def near_coplanar(k, per_face=12):
  """The corners of a box and `per_face` points spread over each of its faces (draws of rock k's stream), turned by
  0.7 + 0.37 k rad about (1 + k, 2, 3 - k / 2), moved off the origin and rounded to float32: the points of a face are coplanar
  to within an ulp or so, and which of them are hull vertices is decided by their roundings.  float64 determinants of float32
  points see those (a triangle of area 1e-4 and a height of 4e-9 give 1e-12, far above float64's 1e-19 here); float32
  determinants (error 3e-12) do not."""
  half = np.array([0.0625, 0.03125, 0.015625])
  i = np.arange(8)
  pts = [(np.stack([(i >> 2) & 1, (i >> 1) & 1, i & 1], axis=1) * 2.0 - 1.0) * half]
  u = draws(k, np.arange(6 * per_face * 2), 5).reshape(6, per_face, 2) * 2.0 - 1.0
  for f in range(6):
    q = np.zeros((per_face, 3))
    q[:, f // 2] = half[f // 2] * (1.0 if f % 2 else -1.0)
    others = [j for j in range(3) if j != f // 2]
    q[:, others] = u[f] * half[others]
    pts.append(q)
  axis = np.array([1.0 + k, 2.0, 3.0 - k / 2.0])
  axis /= np.linalg.norm(axis)
  K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
  angle = 0.7 + 0.37 * k
  R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
  return ((np.concatenate(pts) + [0.011, 0.007, 0.003]) @ R.T).astype(np.float32)


def tetrahedron():
  return np.array([[0.05, 0.01, -0.01], [-0.03, 0.04, 0.0], [-0.02, -0.04, 0.01], [0.0, 0.005, 0.05]], dtype=np.float32)
