"""`srl_render_camera` (include/stackrl_hip.h: scene, camera, rock hit, ground and sky, shading, uint8) restated in numpy, in
float64 or, by argument, in float32 with the kernel's operation order; the scenes and cameras of the camera tests; and the rule
by which an image is held to the float64 restatement.

float32 mode writes a fused multiply-add as the float64 product and sum rounded to float32: the product of two float32 is
exact in float64, so only a sum that lands within 2^-29 of a float32 rounding boundary is rounded differently from the fused
operation — the float32 restatement is the kernel's arithmetic bit for bit but for such a case."""
import numpy as np

from stackrl_amd.camera import Camera
from stackrl_amd.config import MAX_BODIES, StackConfig

F32, F64 = np.float32, np.float64

# Relative depth tolerance where the labels agree: 4 x the largest deviation of the float32 restatement from the float64 one
# over every scene, camera and size of `explicit_cases()` (measured on the CPU by `measure_depth_deviation`, which
# tests/test_camera_cases.py re-runs: 7.44e-6, at the close-up of the grid of 32 bodies, on a face seen at a grazing angle); the factor allows for an operation order that
# differs from this file's but is as legitimate.
DEPTH_MEASURED = 7.44e-6
DEPTH_RTOL = 4 * DEPTH_MEASURED
LABEL_SHARE = 0.005          # of an image's pixels may differ in label, each of them on a border of the float64 labels

SIZES = ((64, 48), (41, 23), (1, 1), (16, 256))      # (width, height): whole tiles; partial both ways, odd; one pixel; tall


def _fma(a, b, c, F):
  if F is F32:
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)
  return a * b + c


def _dot(a, b, F):
  return _fma(a[0], b[0], _fma(a[1], b[1], a[2] * b[2], F), F)


def mesh_planes(pool):
  """Per mesh float32 [nt, 4] — unit face normal and offset in the centre-of-mass frame — and the bounding radius, as
  `srl_load_meshes` makes them (float32, the cross and dot products fused)."""
  out, radii = [], []
  F = F32
  for m in range(len(pool)):
    v, t, mc = pool.mesh(m)
    a = (v.astype(F) - mc[1:4].astype(F)[None]).astype(F)
    A, B, C = a[t[:, 0]], a[t[:, 1]], a[t[:, 2]]
    U, W = B - A, C - A
    n = [_fma(U[:, 1], W[:, 2], -(U[:, 2] * W[:, 1]), F), _fma(U[:, 2], W[:, 0], -(U[:, 0] * W[:, 2]), F),
         _fma(U[:, 0], W[:, 1], -(U[:, 1] * W[:, 0]), F)]
    il = F(1) / np.sqrt(_dot(n, n, F))
    n = [x * il for x in n]
    d = _dot(n, (A[:, 0], A[:, 1], A[:, 2]), F)
    out.append(np.stack(n + [d], -1).astype(F))
    radii.append(float(np.sqrt(_dot(a.T, a.T, F).max())))
  return out, radii


def _rotation(q, F):
  """`quat_to_mat` of the device code: rows of R, each (R_i0, R_i1, R_i2)."""
  x, y, z, w = (F(c) for c in q)
  xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
  one, two = F(1), F(2)
  return ((one - two * (yy + zz), two * (xy - wz), two * (xz + wy)),
          (two * (xy + wz), one - two * (xx + zz), two * (yz - wx)),
          (two * (xz - wy), two * (yz + wx), one - two * (xx + yy)))


def _world_planes(pl, pose, F):
  """(nw [3][nt], dw [nt]) of a body: nw = R . n_f, dw = d_f + dot(nw, x)."""
  R = _rotation(pose[3:7], F)
  n = [pl[:, k].astype(F) for k in range(3)]
  nw = [_fma(R[i][0], n[0], _fma(R[i][1], n[1], R[i][2] * n[2], F), F) for i in range(3)]
  x = [F(pose[k]) for k in range(3)]
  return nw, pl[:, 3].astype(F) + _dot(nw, x, F)


def _clip(nw, num, den):
  """t_in, the face that gave it, t_out, and whether a parallel face shuts the ray out; num, den [nt, P]."""
  with np.errstate(divide='ignore', invalid='ignore'):
    t = num / den
  enter = np.where(den < 0, t, -np.inf)
  tin, fin = enter.max(0), enter.argmax(0)               # (argmax: the first of equals)
  tout = np.where(den > 0, t, np.inf).min(0)
  miss = ((den == 0) & (num < 0)).any(0)
  return tin, fin, tout, miss


def render(planes, poses, mesh_ids, nb, goal, cam, px, res, dtype=F64):
  """One env.  planes: `mesh_planes(pool)[0]`; poses float32 [32, 7+] (position of the centre of mass, quaternion xyzw), mesh_ids
  [32], nb, goal (u, v, h, w); cam: the `srl_camera` struct (`Camera.to_c`); px, res: pixel size and resolution of the overhead
  map.  Returns rgb uint8 [H, W, 3], depth [H, W] (dtype), ids int32 [H, W], and the label map: `shadowed` bool, `zone` (0
  plain or no ground, 1 observable square, 2 goal rectangle) and `labels` = (id + 2) * 8 + shadowed * 4 + zone."""
  F = dtype
  W, H = int(cam.width), int(cam.height)
  vec = lambda a: [F(F32(a[k])) for k in range(3)]
  eye, fwd, right, up, light = vec(cam.eye), vec(cam.fwd), vec(cam.right), vec(cam.up), vec(cam.light)
  s = (2 * np.arange(W) + 1).astype(F) / F(W) - F(1)
  u = F(1) - (2 * np.arange(H) + 1).astype(F) / F(H)
  d = [((fwd[k] + s * right[k])[None, :] + (u * up[k])[:, None]).reshape(-1) for k in range(3)]
  P = H * W
  best, bid = np.full(P, np.inf, F), np.full(P, -1, np.int32)
  nrm = [np.zeros(P, F), np.zeros(P, F), np.ones(P, F)]
  bodies = []
  for b in range(int(nb)):
    nw, dw = _world_planes(planes[int(mesh_ids[b])], poses[b], F)
    bodies.append((nw, dw))
    num = (dw - _dot(nw, eye, F))[:, None]
    den = _dot([c[:, None] for c in nw], [c[None, :] for c in d], F)
    tin, fin, tout, miss = _clip(nw, np.broadcast_to(num, den.shape), den)
    take = ~miss & (tin < tout) & (tin > 0) & (tin < best)     # (slot order: the lower slot keeps a tie)
    best, bid = np.where(take, tin, best), np.where(take, b, bid)
    nrm = [np.where(take, nw[k][fin], nrm[k]) for k in range(3)]
  with np.errstate(divide='ignore', invalid='ignore'):
    tg = np.where(d[2] < 0, -eye[2] / d[2], np.inf).astype(F)
  rock = (bid >= 0) & (best < tg)
  ground = ~rock & (d[2] < 0)
  ids = np.where(rock, bid, np.where(ground, -1, -2)).astype(np.int32)
  t = np.where(rock, best, np.where(ground, tg, np.inf)).astype(F)
  nrm = [np.where(rock, nrm[k], F(k == 2)) for k in range(3)]
  seen = ids != -2
  with np.errstate(invalid='ignore'):
    p = [np.where(seen, _fma(np.where(seen, t, 0), d[k], eye[k], F), 0).astype(F) for k in range(3)]
  lit = np.ones(P, F)
  if cam.shadows and seen.any():
    idx = np.flatnonzero(seen)
    o = [_fma(nrm[k][idx], F(F32(1e-4)), p[k][idx], F) for k in range(3)]
    blocked = np.zeros(len(idx), bool)
    for nw, dw in bodies:
      den = np.broadcast_to(_dot(nw, light, F)[:, None], (len(dw), len(idx)))
      num = dw[:, None] - _dot([c[:, None] for c in nw], [c[None, :] for c in o], F)
      tin, _, tout, miss = _clip(nw, num, den)
      blocked |= ~miss & (tin < tout) & (tout > 0)
    lit[idx[blocked]] = 0
  # shading
  c08, half = F(F32(0.8)), F(F32(0.5))
  sx = F(F32(res) * F32(px))
  g = [F(F32(int(goal[0])) * F32(px)), F(F32(int(goal[0]) + int(goal[2])) * F32(px)),
       F(F32(int(goal[1])) * F32(px)), F(F32(int(goal[1]) + int(goal[3])) * F32(px))]
  obs = ground & (p[0] >= 0) & (p[0] <= sx) & (p[1] >= 0) & (p[1] <= sx)
  ing = obs & (p[0] >= g[0]) & (p[0] <= g[1]) & (p[1] >= g[2]) & (p[1] <= g[3])
  zone = np.where(ing, 2, np.where(obs, 1, 0)).astype(np.int32)
  shade = F(F32(cam.ambient)) + (F(F32(cam.diffuse)) * np.maximum(F(0), _dot(nrm, light, F))) * lit
  rgb = np.zeros((P, 3), F)
  for k in range(3):
    a = np.full(P, c08, F)
    a = np.where(obs, half * a + half, a)
    a = np.where(ing, half * a + (half if k == 1 else F(0)), a)
    a = np.where(rock, F(F32(cam.rock_rgb[k])), a)
    rgb[:, k] = np.where(seen, a * shade, F(F32(cam.sky_rgb[k])))
  rgb8 = np.clip(rgb.astype(F64) * 255 + 0.5, 0, 255).astype(np.uint8)
  shadowed = seen & (lit == 0)
  labels = (ids + 2) * 8 + shadowed * 4 + zone
  return dict(rgb=rgb8.reshape(H, W, 3), depth=t.reshape(H, W), ids=ids.reshape(H, W), shadowed=shadowed.reshape(H, W),
              zone=zone.reshape(H, W), labels=labels.reshape(H, W).astype(np.int32))


def render_batch(planes, scene, cam, config, dtype=F64):
  """`render` over the envs of scene = (poses [B, 32, 7+], mesh_ids [B, 32], nb [B], goal [B, 4]): a list of dicts."""
  poses, mesh_ids, nb, goal = scene
  px, res = F32(config.object_max_dimension) / F32(config.object_res), config.overhead_res
  return [render(planes, poses[e], mesh_ids[e], nb[e], goal[e], cam, px, res, dtype) for e in range(len(nb))]


# ---------------------------------------------------------------------------------------------------- the comparison rule
def border(labels):
  """Pixels with an 8-neighbour of another label."""
  H, W = labels.shape
  pad = np.pad(labels, 1, mode='edge')
  out = np.zeros((H, W), bool)
  for di in range(3):
    for dj in range(3):
      out |= pad[di:di + H, dj:dj + W] != labels
  return out


def depth_deviation(got, ref, where):
  """Largest relative deviation of the finite depths of `where`; inf where one is finite and the other is not."""
  g, r = np.asarray(got['depth'], F64)[where], np.asarray(ref['depth'], F64)[where]
  if g.size == 0:
    return 0.0
  fin = np.isfinite(r)
  if not np.array_equal(fin, np.isfinite(g)) or not np.array_equal(g[~fin], r[~fin]):
    return np.inf
  return float((np.abs(g[fin] - r[fin]) / np.abs(r[fin])).max()) if fin.any() else 0.0


def check(got, ref, tag='', rtol=DEPTH_RTOL):
  """Hold the images `got` (rgb, depth, ids; `labels` too if it has them) to the float64 restatement `ref`.
    - labels may differ in at most 0.5 % of the pixels (none in an image of fewer than 200), each of them with an 8-neighbour
      of another label in `ref`: a silhouette, a shadow edge, a rectangle's border.  Images that come without labels (the
      kernel's) differ in label where their ids differ or, the ids being equal, a colour channel is off by more than 1 level
      — a shadow or a ground zone decided the other way shows as nothing else;
    - where the labels agree rgb is within 1 level per channel and depth within `rtol`, sky being +inf in both.
  Returns the figures (differing pixels, largest depth deviation) for a caller that prints them."""
  ids, rgb = np.asarray(got['ids']), np.asarray(got['rgb']).astype(np.int32)
  assert ids.shape == ref['ids'].shape and rgb.shape == ref['rgb'].shape, tag
  off = np.abs(rgb - ref['rgb'].astype(np.int32)).max(-1)
  if 'labels' in got:
    differ = got['labels'] != ref['labels']
  else:
    differ = (ids != ref['ids']) | (off > 1)
  n, allowed = ids.size, int(LABEL_SHARE * ids.size)
  stray = differ & ~border(ref['labels'])
  assert not stray.any(), '{}: {} pixels differ away from every border of the labels, first at {}'.format(
    tag, int(stray.sum()), np.argwhere(stray)[0].tolist())
  assert differ.sum() <= allowed, '{}: {} of {} pixels differ in label, {} allowed'.format(tag, int(differ.sum()), n, allowed)
  agree = ~differ
  assert np.array_equal(ids[agree], ref['ids'][agree]), tag
  worst = int(off[agree].max()) if agree.any() else 0
  assert worst <= 1, '{}: a colour channel is off by {} levels at {} (labels agree)'.format(tag, worst, np.argwhere(agree & (off > 1))[0].tolist())
  dev = depth_deviation(got, ref, agree)
  assert dev <= rtol, '{}: depth deviates by {:.3e} (relative) where the labels agree, {:.3e} allowed'.format(tag, dev, rtol)
  return int(differ.sum()), dev


# ---------------------------------------------------------------------------------------------------- scenes and cameras
CONFIG = StackConfig()        # the default env: 128 x 128 overhead map of 0.5 m x 0.5 m, max_z 0.375


def _quat(rng):
  q = rng.normal(size=4)
  return (q / np.linalg.norm(q)).astype(F32)


def empty_scene(B):
  return (np.zeros((B, MAX_BODIES, 7), F32), np.zeros((B, MAX_BODIES), np.int32), np.zeros(B, np.int32), np.zeros((B, 4), np.int32))


def goals(B, res=128, h=32):
  """A different goal per env: env 0's starts in the first row and column, env 1's ends in the last."""
  rect = np.zeros((B, 4), np.int32)
  for e in range(B):
    gh, gw = h + 8 * e, 2 * h - 4 * e
    u, v = (0, 0) if e == 0 else (res - gh, res - gw) if e == 1 else (res // 3, res // 4)
    rect[e] = (u, v, gh, gw)
  return rect


def pile_scene(pool, B, n=5, seed=0):
  """n rocks per env tumbled over the middle of the observable square, some resting on the ground plane's height, some above."""
  rng = np.random.RandomState(seed)
  poses, mesh, nb, _ = empty_scene(B)
  for e in range(B):
    k = max(1, n - e)
    nb[e] = k
    mesh[e, :k] = rng.choice(len(pool), size=k, replace=False)
    for b in range(k):
      poses[e, b, :3] = (0.25 + rng.uniform(-0.09, 0.09), 0.25 + rng.uniform(-0.09, 0.09), 0.035 + 0.03 * b + rng.uniform(0, 0.01))
      poses[e, b, 3:] = _quat(rng)
  return poses, mesh, nb, goals(B)


def grid_scene(pool, B, seed=1):
  """32 bodies per env on a 6 x 6 grid over the square, in two heights, the pool's mesh with the most faces among them."""
  rng = np.random.RandomState(seed)
  most = int(np.argmax(np.diff(pool.tri_off)))
  poses, mesh, nb, _ = empty_scene(B)
  for e in range(B):
    nb[e] = MAX_BODIES
    mesh[e] = rng.randint(0, len(pool), size=MAX_BODIES)
    mesh[e, (5 + 7 * e) % MAX_BODIES] = most
    for b in range(MAX_BODIES):
      poses[e, b, :3] = (0.06 + 0.075 * (b % 6) + rng.uniform(-0.01, 0.01), 0.06 + 0.075 * (b // 6) + rng.uniform(-0.01, 0.01),
                         0.04 + 0.08 * ((b + e) % 2))
      poses[e, b, 3:] = _quat(rng)
  return poses, mesh, nb, goals(B)


def coincident_scene(pool, B, seed=2):
  """Slots 1 and 2 hold the same rock at the same pose (slot 1 is seen), slot 0 another rock beside them."""
  rng = np.random.RandomState(seed)
  poses, mesh, nb, _ = empty_scene(B)
  for e in range(B):
    nb[e] = 3
    a, c = rng.choice(len(pool), size=2, replace=False)
    mesh[e, :3] = (a, c, c)
    poses[e, 0, :3] = (0.16, 0.3, 0.05)
    poses[e, 0, 3:] = _quat(rng)
    poses[e, 1, :3] = (0.3 + 0.01 * e, 0.22, 0.06)
    poses[e, 1, 3:] = _quat(rng)
    poses[e, 2] = poses[e, 1]
  return poses, mesh, nb, goals(B)


def cameras(config=CONFIG):
  return {
    'reference': Camera.reference(config),
    'closeup': Camera.look_at((0.25, 0.25, 0.08), 0.3, 30., -25.),
    'up': Camera.look_at((0.25, 0.25, 0.0), 0.8, 45., 40.),
    'noshadow': Camera.reference(config, shadows=False),
  }


def explicit_cases(pool):
  """(tag, scene builder B -> scene, camera name, (width, height)) of every explicit scene the GPU suite renders."""
  scenes = {'empty': lambda B: empty_scene(B)[:3] + (goals(B),), 'pile': lambda B: pile_scene(pool, B), 'grid': lambda B: grid_scene(pool, B),
            'coincident': lambda B: coincident_scene(pool, B)}
  cases = []
  for size in SIZES:
    cases += [('pile', 'reference', size), ('pile', 'noshadow', size)]
  cases += [('empty', 'reference', (64, 48)), ('grid', 'reference', (41, 23)), ('grid', 'closeup', (64, 48)),
            ('coincident', 'reference', (64, 48)), ('coincident', 'closeup', (41, 23)), ('pile', 'closeup', (64, 48)),
            ('pile', 'up', (41, 23)), ('pile', 'closeup', (16, 256))]
  return [('{} {} {}x{}'.format(s, c, *size), scenes[s], c, size) for s, c, size in cases]


def measure_depth_deviation(pool, planes, B=3):
  """The largest relative deviation of the float32 restatement's depths from the float64 one's over `explicit_cases`, where
  their labels agree: what DEPTH_MEASURED records."""
  worst, cams = 0.0, cameras()
  for tag, scene, cam, (w, h) in explicit_cases(pool):
    c = cams[cam].to_c(w, h)
    sc = scene(B)
    for r32, r64 in zip(render_batch(planes, sc, c, CONFIG, F32), render_batch(planes, sc, c, CONFIG, F64)):
      worst = max(worst, depth_deviation(r32, r64, r32['labels'] == r64['labels']))
  return worst
