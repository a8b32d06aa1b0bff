"""CPU tests of the camera view's definition (tests/camera_cases.py restates include/stackrl_hip.h's text for
`srl_render_camera`) and of `stackrl_amd.camera.Camera`: closed forms the restatement must reproduce, and the conditions under
which tests/test_camera_gpu.py holds the kernel to it."""
import math

import numpy as np
import pytest

import camera_cases as cc
from stackrl_amd import assets
from stackrl_amd.camera import Camera

CFG = cc.CONFIG


@pytest.fixture(scope='module')
def ref_planes(ref_pool):
  return cc.mesh_planes(ref_pool)[0]


@pytest.fixture(scope='module')
def box():
  """A pool of one cuboid, its planes and its half extents."""
  pool = assets.pack([assets.cuboid()])
  return pool, cc.mesh_planes(pool)[0], pool.mesh(0)[0].astype(np.float64).max(0)


def _scene(bodies, goal=(40, 30, 32, 48)):
  """One env of explicit bodies [(mesh, position, quaternion)]."""
  poses, mesh, nb, rect = cc.empty_scene(1)
  for b, (m, x, q) in enumerate(bodies):
    poses[0, b, :3], poses[0, b, 3:], mesh[0, b] = x, q, m
  nb[0], rect[0] = len(bodies), goal
  return poses, mesh, nb, rect


def _render(planes, scene, cam, w, h, dtype=cc.F64):
  return cc.render_batch(planes, scene, cam.to_c(w, h), CFG, dtype)[0]


def _hit_points(cam, w, h, depth):
  """World points eye + t d of every pixel, in float64 from the struct's values."""
  c = cam.to_c(w, h)
  v = lambda a: np.array([a[0], a[1], a[2]], np.float64)
  s = (2 * np.arange(w) + 1) / w - 1
  u = 1 - (2 * np.arange(h) + 1) / h
  d = v(c.fwd)[None, None] + s[None, :, None] * v(c.right)[None, None] + u[:, None, None] * v(c.up)[None, None]
  with np.errstate(invalid='ignore'):
    return v(c.eye)[None, None] + np.asarray(depth, np.float64)[..., None] * d


def _project(cam, w, h, pts):
  """Fractional (row, column) of world points."""
  rel = np.asarray(pts, np.float64) - np.asarray(cam.eye)[None]
  z = rel @ np.asarray(cam.fwd)
  th = math.tan(math.radians(cam.fov) / 2)
  s = (rel @ np.asarray(cam.right)) / (z * th * w / h)
  u = (rel @ np.asarray(cam.up)) / (z * th)
  return ((1 - u) * h - 1) / 2, ((s + 1) * w - 1) / 2


IDENT = (0., 0., 0., 1.)


def test_look_at_gives_an_orthonormal_frame_and_the_reference_view():
  cam = Camera.look_at((0.1, 0.2, 0.3), 2.0, 30., -20., fov=50.)
  f, r, u = (np.array(x) for x in (cam.fwd, cam.right, cam.up))
  for a in (f, r, u):
    assert abs(np.linalg.norm(a) - 1) < 1e-12
  assert abs(f @ r) < 1e-12 and abs(f @ u) < 1e-12 and abs(r @ u) < 1e-12 and np.allclose(np.cross(r, f), u)
  assert u[2] > 0 and f[2] < 0 and np.allclose(np.array(cam.eye) + 2.0 * f, (0.1, 0.2, 0.3))
  c = cam.to_c(320, 240)
  th = math.tan(math.radians(25.))
  assert np.allclose(np.array(c.right[:]), r * th * 320 / 240, rtol=1e-6) and np.allclose(np.array(c.up[:]), u * th, rtol=1e-6)
  assert abs(np.linalg.norm(np.array(c.light[:])) - 1) < 1e-6 and (c.width, c.height, c.shadows) == (320, 240, 1)
  ref = Camera.reference(CFG)
  dist = math.sqrt(0.5 ** 2 + 0.5 ** 2 + 0.375 ** 2)      # env.py:275-281 on `Observer.size` of the default env
  assert np.allclose(ref.eye, (0.25 + dist / 2, 0.25 - dist / 2, dist * math.sin(math.radians(45))), atol=1e-12) and ref.fov == 60.
  with pytest.raises(ValueError):
    Camera.look_at((0, 0, 0), 1., 0., 90.)


def test_the_centre_ray_of_the_reference_view_meets_the_ground_at_the_target(ref_planes):
  cam = Camera.reference(CFG)
  sx = CFG.overhead_res * CFG.pixel_size
  dist = math.sqrt(2 * sx * sx + CFG.max_z ** 2)
  for w, h in ((33, 25), (1, 1), (41, 23)):
    out = _render(ref_planes, cc.empty_scene(1), cam, w, h)
    i, j = h // 2, w // 2
    assert out['ids'][i, j] == -1 and abs(out['depth'][i, j] - dist) < 1e-6 * dist
    assert np.allclose(_hit_points(cam, w, h, out['depth'])[i, j], (sx / 2, sx / 2, 0.), atol=1e-6)
    assert (out['ids'] == -1).all() and not out['shadowed'].any()


def test_a_cuboid_on_the_centre_ray_is_met_at_the_analytic_depth_and_fills_its_projection(box):
  pool, planes, half = box
  cam = Camera.reference(CFG)
  dist = math.sqrt(0.5 + CFG.max_z ** 2)
  top = np.array((0.25, 0.25, 0.)) - 0.2 * np.array(cam.fwd)          # the top face's centre, 0.2 m up the centre ray
  centre = top - (0, 0, half[2])
  w, h = 65, 49
  out = _render(planes, _scene([(0, centre, IDENT)]), cam, w, h)
  i, j = h // 2, w // 2
  assert out['ids'][i, j] == 0 and abs(out['depth'][i, j] - (dist - 0.2)) < 1e-6
  assert np.allclose(_hit_points(cam, w, h, out['depth'])[i, j], top, atol=1e-6)
  # the up-facing normal: the centre pixel has the lit colour of a face whose normal is +z
  c = cam.to_c(w, h)
  shade = c.ambient + c.diffuse * c.light[2]
  want = [int(np.clip(c.rock_rgb[k] * shade * 255 + 0.5, 0, 255)) for k in range(3)]
  assert np.abs(out['rgb'][i, j].astype(int) - want).max() <= 1
  # the mask's bounding box is that of the projected vertices, within one pixel
  verts = pool.mesh(0)[0].astype(np.float64) + centre[None]
  rows, cols = _project(cam, w, h, verts)
  mi, mj = np.nonzero(out['ids'] == 0)
  for got, want in ((mi.min(), rows.min()), (mi.max(), rows.max()), (mj.min(), cols.min()), (mj.max(), cols.max())):
    assert abs(got - want) <= 1, (got, want)
  # a rotated cuboid: a quarter turn about z swaps its x and y extents
  q = (0., 0., math.sin(math.pi / 4), math.cos(math.pi / 4))
  out = _render(planes, _scene([(0, centre, q)]), cam, w, h)
  R = np.array(((0., -1., 0.), (1., 0., 0.), (0., 0., 1.)))
  rows, cols = _project(cam, w, h, pool.mesh(0)[0].astype(np.float64) @ R.T + centre[None])
  mi, mj = np.nonzero(out['ids'] == 0)
  for got, want in ((mi.min(), rows.min()), (mi.max(), rows.max()), (mj.min(), cols.min()), (mj.max(), cols.max())):
    assert abs(got - want) <= 1, (got, want)
  assert out['ids'][i, j] == 0 and abs(out['depth'][i, j] - (dist - 0.2)) < 1e-6


def test_the_nearer_of_two_rocks_in_line_is_seen_and_the_lower_slot_of_two_coincident_ones(box, ref_pool, ref_planes):
  pool, planes, half = box
  cam = Camera.reference(CFG)
  w, h = 33, 25
  i, j = h // 2, w // 2
  near = np.array((0.25, 0.25, 0.)) - 0.3 * np.array(cam.fwd)
  far = np.array((0.25, 0.25, 0.)) - 0.1 * np.array(cam.fwd)
  seen = []
  for order in ((near, far), (far, near)):
    out = _render(planes, _scene([(0, order[0], IDENT), (0, order[1], IDENT)]), cam, w, h)
    assert out['ids'][i, j] == (0 if order[0] is near else 1)
    seen.append(out)
  swapped = np.where(seen[1]['ids'] >= 0, 1 - seen[1]['ids'], seen[1]['ids'])      # the same picture whichever slot is which
  assert np.array_equal(seen[0]['ids'], swapped) and np.array_equal(seen[0]['rgb'], seen[1]['rgb'])
  out = _render(planes, _scene([(0, near, IDENT), (0, near, IDENT), (0, near, IDENT)]), cam, w, h)
  assert set(np.unique(out['ids'])) == {-1, 0}
  for e, out in enumerate(cc.render_batch(ref_planes, cc.coincident_scene(ref_pool, 3), cc.cameras()['closeup'].to_c(64, 48), CFG)):
    assert (out['ids'] == 1).sum() > 50 and not (out['ids'] == 2).any(), e


def test_a_floating_cuboid_under_a_vertical_light_shades_its_own_rectangle_of_the_ground(box):
  pool, planes, half = box
  cam = Camera.reference(CFG, light=(0., 0., 1.))
  centre = np.array((0.27, 0.22, 0.3))
  w, h = 128, 96
  out = _render(planes, _scene([(0, centre, IDENT)]), cam, w, h)
  ground = out['ids'] == -1
  p = _hit_points(cam, w, h, out['depth'])
  assert np.abs(p[ground][:, 2]).max() < 1e-6
  # half a pixel's footprint on the ground: half the distance to the farthest of the four neighbours' hit points
  pad = np.pad(p[..., :2], ((1, 1), (1, 1), (0, 0)), mode='edge')
  step = np.zeros((h, w))
  for di, dj in ((0, 1), (2, 1), (1, 0), (1, 2)):
    step = np.maximum(step, np.linalg.norm(pad[di:di + h, dj:dj + w] - p[..., :2], axis=-1))
  lo, hi = centre[:2] - half[:2], centre[:2] + half[:2]
  inside = ((p[..., :2] >= lo) & (p[..., :2] <= hi)).all(-1)
  away = np.maximum(np.maximum(lo - p[..., :2], p[..., :2] - hi), 0)
  to_edge = np.where(inside, np.minimum(p[..., :2] - lo, hi - p[..., :2]).min(-1), np.linalg.norm(away, axis=-1))
  clear = ground & (to_edge > step / 2)
  assert (clear & inside).sum() > 20 and (clear & ~inside).sum() > 1000
  assert out['shadowed'][clear & inside].all() and not out['shadowed'][clear & ~inside].any()
  # the cuboid's top is lit, its sides and its underside are not (a vertical light grazes or misses them)
  top = (out['ids'] == 0) & (np.abs(p[..., 2] - (centre[2] + half[2])) < 1e-5)
  assert top.sum() > 20 and not out['shadowed'][top].any()
  # without shadows nothing is
  assert not _render(planes, _scene([(0, centre, IDENT)]), Camera.reference(CFG, light=(0., 0., 1.), shadows=False), w, h)['shadowed'].any()


def test_zone_colours_of_the_ground(ref_planes):
  cam = Camera.look_at((0.25, 0.25, 0.), 1.2, 45., -60., shadows=False)
  w, h = 80, 60
  goal = (40, 30, 32, 48)
  out = _render(ref_planes, _scene([], goal), cam, w, h)
  assert (out['ids'] == -1).all()
  p = _hit_points(cam, w, h, out['depth'])
  px, sx = CFG.pixel_size, CFG.overhead_res * CFG.pixel_size
  eps = 1e-6
  obs = ((p[..., :2] > eps) & (p[..., :2] < sx - eps)).all(-1)
  out_obs = ((p[..., :2] < -eps) | (p[..., :2] > sx + eps)).any(-1)
  x0, x1, y0, y1 = goal[0] * px, (goal[0] + goal[2]) * px, goal[1] * px, (goal[1] + goal[3]) * px
  ing = (p[..., 0] > x0 + eps) & (p[..., 0] < x1 - eps) & (p[..., 1] > y0 + eps) & (p[..., 1] < y1 - eps)
  out_goal = (p[..., 0] < x0 - eps) | (p[..., 0] > x1 + eps) | (p[..., 1] < y0 - eps) | (p[..., 1] > y1 + eps)
  assert (out['zone'][ing] == 2).all() and (out['zone'][obs & out_goal] == 1).all() and (out['zone'][out_obs] == 0).all()
  assert ing.sum() > 20 and (obs & out_goal).sum() > 200 and out_obs.sum() > 500
  c = cam.to_c(w, h)
  shade = c.ambient + c.diffuse * c.light[2]
  for zone, albedo in ((0, (0.8, 0.8, 0.8)), (1, (0.9, 0.9, 0.9)), (2, (0.45, 0.95, 0.45))):
    want = np.array([int(np.clip(a * shade * 255 + 0.5, 0, 255)) for a in albedo])
    got = out['rgb'][out['zone'] == zone].astype(int)
    assert np.abs(got - want[None]).max() <= 1, zone


def test_a_camera_pitched_above_the_horizon_sees_sky(ref_pool, ref_planes):
  cam = cc.cameras()['up']
  out = _render(ref_planes, cc.empty_scene(1), cam, 41, 23)
  assert (out['ids'] == -2).all() and np.isposinf(out['depth']).all() and not out['shadowed'].any()
  c = cam.to_c(41, 23)
  want = [int(np.clip(np.float64(c.sky_rgb[k]) * 255 + 0.5, 0, 255)) for k in range(3)]
  assert (out['rgb'] == np.array(want, np.uint8)[None, None]).all()
  # rocks that float into the view are seen against it
  out = cc.render_batch(ref_planes, cc.pile_scene(ref_pool, 1), c, CFG)[0]
  assert set(np.unique(out['ids'])) >= {-2, 0} and -1 not in out['ids']
  assert np.isposinf(out['depth'][out['ids'] == -2]).all() and np.isfinite(out['depth'][out['ids'] >= 0]).all()


def test_the_float32_restatement_meets_the_comparison_rule_on_every_explicit_case_of_the_gpu_suite(ref_pool, ref_planes):
  """The conditions of the GPU suite: the rule's caps must be met by the inputs themselves, so every explicit scene, camera
  and size tests/test_camera_gpu.py renders goes through the float32 restatement here and is held to the float64 one — with
  its own labels, which the kernel's images do not carry.  (The scenes of an env's own state exist only on the device: the GPU
  tests put each of them through this same check before they look at the kernel's images.)  The depth tolerance is 4 x the
  largest deviation measured here."""
  cams, worst = cc.cameras(), 0.0
  for tag, scene, cam, (w, h) in cc.explicit_cases(ref_pool):
    c = cams[cam].to_c(w, h)
    for B in (1, 3):
      sc = scene(B)
      for e, (r32, r64) in enumerate(zip(cc.render_batch(ref_planes, sc, c, CFG, cc.F32), cc.render_batch(ref_planes, sc, c, CFG, cc.F64))):
        differ, dev = cc.check(r32, r64, '{} B = {} env {}'.format(tag, B, e), rtol=cc.DEPTH_MEASURED * 1.0005)
        worst = max(worst, dev)
  print('largest relative depth deviation of float32 from float64: {:.3e}'.format(worst))
  assert 0.98 * cc.DEPTH_MEASURED <= worst <= cc.DEPTH_MEASURED * 1.0005 and cc.DEPTH_RTOL == 4 * cc.DEPTH_MEASURED


def test_the_rule_tells_wrong_images_apart(ref_pool, ref_planes):
  """`check` refuses: a shifted image, a label off a border, too many labels on borders, a colour off by two, a depth off."""
  c = cc.cameras()['reference'].to_c(64, 48)
  ref = cc.render_batch(ref_planes, cc.pile_scene(ref_pool, 1), c, CFG)[0]
  same = {k: ref[k].copy() for k in ('rgb', 'depth', 'ids')}
  assert cc.check(same, ref) == (0, 0.0)
  bad = dict(same, ids=np.roll(ref['ids'], 1, axis=1), rgb=np.roll(ref['rgb'], 1, axis=1), depth=np.roll(ref['depth'], 1, axis=1))
  with pytest.raises(AssertionError, match='pixels differ'):
    cc.check(bad, ref)
  flat = np.argwhere(~cc.border(ref['labels']) & (ref['ids'] == -1))[0]
  bad = dict(same, ids=ref['ids'].copy())
  bad['ids'][tuple(flat)] = 0
  with pytest.raises(AssertionError, match='away from every border'):
    cc.check(bad, ref)
  bad = dict(same, rgb=ref['rgb'].copy())
  bad['rgb'][tuple(flat)] += 2
  with pytest.raises(AssertionError, match='away from every border'):
    cc.check(bad, ref)
  bad = dict(same, depth=ref['depth'] * np.float64(1 + 2 * cc.DEPTH_RTOL))
  with pytest.raises(AssertionError, match='depth deviates'):
    cc.check(bad, ref)
  edge = np.argwhere(cc.border(ref['labels']))
  bad = dict(same, ids=ref['ids'].copy())
  for q in edge[:int(cc.LABEL_SHARE * ref['ids'].size) + 1]:
    bad['ids'][tuple(q)] = 7
  with pytest.raises(AssertionError, match='allowed'):
    cc.check(bad, ref)
  # an image of fewer than 200 pixels: none may differ
  small = cc.render_batch(ref_planes, cc.pile_scene(ref_pool, 1), cc.cameras()['reference'].to_c(13, 11), CFG)[0]
  bad = {k: small[k].copy() for k in ('rgb', 'depth', 'ids')}
  q = tuple(np.argwhere(cc.border(small['labels']))[0])
  bad['ids'][q] = 9
  with pytest.raises(AssertionError, match='0 allowed'):
    cc.check(bad, small)
