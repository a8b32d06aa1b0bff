"""GPU tests of `render_camera` (csrc/camera.hip behind `srl_render_camera`): the kernel's images are held to the float64
restatement of the definition (tests/camera_cases.py) by the comparison rule there — labels differ in at most 0.5 % of the
pixels and only on borders of the float64 labels, rgb within one level and depth within DEPTH_RTOL where they agree.

Sizes: a tile is 32 x 8 pixels, a wave two rows of it.  64 x 48 is whole tiles; 41 x 23 has partial tiles both ways (the last
wave of the last tile row owns one row, the last tile column 9 of 32 columns); 1 x 1 is one lane; 16 x 256 half a tile wide.
Scenes: nothing placed, an env's own state through an episode, 32 bodies (staged a few at a time: several chunks, and again for the
shadows), two coincident rocks; B = 1 and 3 with other rocks and goals per env."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import camera_cases as cc

pytestmark = pytest.mark.gpu

CFG = cc.CONFIG
_cache = {}


def _planes(pool):
  if 'planes' not in _cache:
    _cache['planes'] = cc.mesh_planes(pool)[0]
  return _cache['planes']


def _env(pool, B, **kw):
  from stackrl_amd import env as envs
  kw.setdefault('episode_length', 3)
  return envs.VecStackEnv(n_parallel=B, seed=3, pool=pool, block=True, **kw)


def _images(g, cam, w, h, scene=None):
  """The kernel's three images, per env, as numpy."""
  rgb, depth, ids = g.render_camera(w, h, camera=cam, rgb=True, depth=True, ids=True, scene=scene)
  assert rgb.dtype == torch.uint8 and depth.dtype == torch.float32 and ids.dtype == torch.int32
  assert tuple(rgb.shape) == (g.batch_size, h, w, 3) and tuple(depth.shape) == tuple(ids.shape) == (g.batch_size, h, w)
  rgb, depth, ids = rgb.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()
  return [dict(rgb=rgb[e], depth=depth[e], ids=ids[e]) for e in range(g.batch_size)]


def _hold(got, refs, tag):
  for e, (a, r) in enumerate(zip(got, refs)):
    differ, dev = cc.check(a, r, '{} env {}'.format(tag, e))
    print('{} env {}: {} pixels differ in label, depth deviates by {:.2e}'.format(tag, e, differ, dev))


def _script(env, pool, seed):
  """Different rocks and a different goal per env."""
  B, L = env.batch_size, env.config.episode_length
  rng = np.random.RandomState(seed)
  ids = np.stack([rng.choice(len(pool), size=L, replace=False) for _ in range(B)]).astype(np.int32)
  rect = cc.goals(B)
  env.set_script(ids, rect)
  return rect


def _pixels(env, k):
  """Placements near the centre of the action map, another pixel per env and step, so that the rocks pile up."""
  AW = env.config.overhead_res - env.config.object_res + 1
  i = AW // 2 + (np.arange(env.batch_size) * 3 + k * 5) % 7 - 3
  j = AW // 2 - (np.arange(env.batch_size) * 2 + k * 3) % 5 + 2
  return torch.as_tensor(i * AW + j, dtype=torch.int64)


def _own_scene(g):
  """The env's own state as the restatement takes it: `state()` and `maps()[2]`."""
  poses, nb, _, _ = g.state()
  return poses, poses[:, :, 7].astype(np.int32), nb, g.maps()[2]


CASES = None


def _cases(pool):
  global CASES
  if CASES is None:
    CASES = {tag: (scene, cam, size) for tag, scene, cam, size in cc.explicit_cases(pool)}
  return CASES


def _case_tags():
  return [c[0] for c in cc.explicit_cases(None)]      # (the tags do not depend on the pool; the scenes are built later)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('tag', _case_tags())
def test_explicit_scenes(ref_pool, tag, B):
  """Every explicit scene, camera and size of `camera_cases.explicit_cases` (tests/test_camera_cases.py holds the float32
  restatement to the rule on each of them: the rule's conditions)."""
  scene, cam, (w, h) = _cases(ref_pool)[tag]
  cam, sc = cc.cameras()[cam], scene(B)
  g = _env(ref_pool, B)
  try:
    got = _images(g, cam, w, h, scene=sc)
  finally:
    g.close()
  refs = cc.render_batch(_planes(ref_pool), sc, cam.to_c(w, h), CFG)
  _hold(got, refs, tag)
  if tag.startswith('coincident'):
    assert all((a['ids'] == 1).any() and not (a['ids'] == 2).any() for a in got)
  if tag.startswith('pile up'):
    assert all(np.isposinf(a['depth'][a['ids'] == -2]).all() and (a['ids'] == -2).sum() > 300 for a in got)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('size', [(64, 48), (41, 23)])
def test_the_envs_own_state_through_an_episode(ref_pool, size, B):
  """Before the first reset (nothing placed), after the reset, after each of 3 placements and after the auto-reset, with and
  without shadows.  These scenes exist only on the device, so the rule's conditions are checked here: the float32
  restatement of each must meet the rule before the kernel's images are looked at."""
  w, h = size
  planes = _planes(ref_pool)
  cams = cc.cameras()
  g = _env(ref_pool, B)

  def look(tag, placed):
    sc = _own_scene(g)
    assert (sc[2] == placed).all()
    for name in ('reference', 'noshadow'):
      c = cams[name].to_c(w, h)
      r64, r32 = cc.render_batch(planes, sc, c, CFG), cc.render_batch(planes, sc, c, CFG, cc.F32)
      for e in range(B):
        cc.check(r32[e], r64[e], 'condition: {} {} env {}'.format(tag, name, e))
      _hold(_images(g, cams[name], w, h), r64, '{} {}'.format(tag, name))
    return r64

  try:
    r = look('new', 0)
    assert all((x['ids'] == -1).all() for x in r)
    rect = _script(g, ref_pool, 5)
    g.reset()
    r = look('reset', 0)
    assert np.array_equal(g.maps()[2], rect) and all((x['zone'] == 2).any() for x in r)
    for k in range(3):
      g.step(_pixels(g, k))
      r = look('step {}'.format(k), k + 1)
      assert all((x['ids'] == k).any() for x in r)
    g.step(_pixels(g, 0))                                # env.py:235-236: the auto-reset
    look('auto-reset', 0)
  finally:
    g.close()


def test_every_combination_of_outputs(ref_pool):
  g = _env(ref_pool, 2)
  try:
    sc, cam = cc.pile_scene(ref_pool, 2), cc.cameras()['reference']
    full = g.render_camera(41, 23, camera=cam, rgb=True, depth=True, ids=True, scene=sc)
    for mask in range(1, 8):
      want = [bool(mask & 1), bool(mask & 2), bool(mask & 4)]
      got = g.render_camera(41, 23, camera=cam, rgb=want[0], depth=want[1], ids=want[2], scene=sc)
      got = got if isinstance(got, tuple) else (got,)
      assert len(got) == sum(want)
      for t, f in zip(got, [f for f, on in zip(full, want) if on]):
        assert torch.equal(t, f), mask
    assert torch.equal(g.render_camera(41, 23, camera=cam, scene=sc), full[0])      # rgb alone is the default
    with pytest.raises(ValueError, match='srl_render_camera: all outputs are NULL'):
      g.render_camera(41, 23, camera=cam, rgb=False, scene=sc)
  finally:
    g.close()


def test_out_tensors_are_filled_in_place(ref_pool):
  B, w, h = 2, 41, 23
  g = _env(ref_pool, B)
  try:
    sc, cam = cc.pile_scene(ref_pool, B), cc.cameras()['reference']
    full = g.render_camera(w, h, camera=cam, rgb=True, depth=True, ids=True, scene=sc)
    big = (torch.full((B + 2, h, w, 3), 7, dtype=torch.uint8, device='cuda'), torch.full((B + 2, h, w), 7, dtype=torch.float32, device='cuda'),
           torch.full((B + 2, h, w), 7, dtype=torch.int32, device='cuda'))
    out = [t[1:1 + B] for t in big]
    got = g.render_camera(w, h, camera=cam, rgb=True, depth=True, ids=True, out=out, scene=sc)
    for k in range(3):
      assert got[k] is out[k] and torch.equal(big[k][1:1 + B], full[k])
      assert bool((big[k][0] == 7).all() and (big[k][-1] == 7).all())
    # rgb that starts one byte into a line, with a guard byte on either side
    n = B * h * w * 3
    flat = torch.full((n + 2,), 7, dtype=torch.uint8, device='cuda')
    view = flat[1:1 + n].view(B, h, w, 3)
    assert g.render_camera(w, h, camera=cam, out=view, scene=sc) is view
    assert torch.equal(view, full[0]) and int(flat[0]) == 7 and int(flat[-1]) == 7
    with pytest.raises(ValueError, match='out must be'):
      g.render_camera(w, h, camera=cam, out=torch.empty((B, h, w, 3), dtype=torch.float32, device='cuda'), scene=sc)
    with pytest.raises(ValueError, match='one tensor per image'):
      g.render_camera(w, h, camera=cam, depth=True, out=view, scene=sc)
  finally:
    g.close()


def test_a_view_right_after_a_step_that_was_not_waited_for(ref_pool):
  """side_stream: `render_camera` right after a non-blocking `step` is ordered after that step's kernels: it shows its poses."""
  from stackrl_amd import env as envs
  B, w, h = 3, 64, 48
  g = envs.VecStackEnv(n_parallel=B, seed=3, pool=ref_pool, block=False, episode_length=3, side_stream=True)
  try:
    _script(g, ref_pool, 19)
    g.reset()()
    cam = cc.cameras()['reference']
    before = g.render_camera(w, h, camera=cam, ids=True, rgb=False).clone()
    wait = g.step(_pixels(g, 0))
    rgb, depth, ids = g.render_camera(w, h, camera=cam, rgb=True, depth=True, ids=True)      # the step has not been waited for
    wait()
    assert not (before >= 0).any() and all(bool((ids[e] == 0).any()) for e in range(B))
    refs = cc.render_batch(_planes(ref_pool), _own_scene(g), cam.to_c(w, h), CFG)
    _hold([dict(rgb=rgb[e].cpu().numpy(), depth=depth[e].cpu().numpy(), ids=ids[e].cpu().numpy()) for e in range(B)], refs, 'side stream')
  finally:
    g.close()


def test_the_pipelined_env_is_its_groups_in_env_order(ref_pool):
  from stackrl_amd import env as envs
  B, w, h = 4, 41, 23
  g = envs.PipelinedVecStackEnv(n_parallel=B, groups=2, seed=3, pool=ref_pool, block=True, episode_length=3)
  try:
    _script(g, ref_pool, 23)
    g.reset()
    g.step(_pixels(g, 0))
    cam = cc.cameras()['closeup']
    got = g.render_camera(w, h, camera=cam, rgb=True, depth=True, ids=True)
    parts = [e.render_camera(w, h, camera=cam, rgb=True, depth=True, ids=True) for e in g._envs]
    for k in range(3):
      assert torch.equal(got[k], torch.cat([p[k] for p in parts]))
    assert tuple(got[0].shape) == (B, h, w, 3) and bool((got[2] == 0).any())
    one = g.render_camera(w, h, camera=cam)
    assert torch.is_tensor(one) and torch.equal(one, got[0])
    poses, nb, _, _ = g.state()
    refs = cc.render_batch(_planes(ref_pool), (poses, poses[:, :, 7].astype(np.int32), nb, g.maps()[2]), cam.to_c(w, h), CFG)
    _hold([dict(rgb=got[0][e].cpu().numpy(), depth=got[1][e].cpu().numpy(), ids=got[2][e].cpu().numpy()) for e in range(B)], refs, 'pipelined')
    with pytest.raises(ValueError, match='width and height must be in 1 .. 1024'):
      g.render_camera(0, 10)
    with pytest.raises(ValueError, match="Only 'rgb_array' is supported"):
      g.render('human')
  finally:
    g.close()


def test_the_started_env_inherits_the_method(ref_pool):
  from stackrl_amd import env as envs
  g = envs.make('Stack-v1', n_parallel=2, seed=3, pool=ref_pool, block=True, episode_length=2, n_objects=4)
  try:
    g.reset()                                            # two rocks placed by the start policy
    cam, (w, h) = cc.cameras()['reference'], (64, 48)
    sc = _own_scene(g)
    assert (sc[2] == 2).all()
    refs = cc.render_batch(_planes(ref_pool), sc, cam.to_c(w, h), CFG)
    _hold(_images(g, cam, w, h), refs, 'started')
    assert all((r['ids'] == 1).any() for r in refs)
  finally:
    g.close()


def test_every_refusal_in_its_own_words(ref_pool):
  from stackrl_amd.camera import Camera
  g = _env(ref_pool, 1)
  try:
    cam = cc.cameras()['reference']
    for w, h in ((0, 10), (10, 0), (1025, 10), (10, 1025), (-3, 5)):
      with pytest.raises(ValueError, match=r'srl_render_camera: width and height must be in 1 \.\. 1024'):
        g.render_camera(w, h, camera=cam)
    for bad in (Camera.look_at((float('nan'), 0, 0), 1., 0., -30.), Camera.reference(CFG, ambient=float('inf')),
                Camera.reference(CFG, sky_rgb=(0.5, float('nan'), 0.5))):
      with pytest.raises(ValueError, match='srl_render_camera: the camera holds a non-finite value'):
        g.render_camera(16, 8, camera=bad)
    rgb = torch.empty((1, 8, 16, 3), dtype=torch.uint8, device='cuda')
    for field, scale in (('fwd', 1.002), ('light', 0.998), ('fwd', 0.0)):
      c = cam.to_c(16, 8)
      setattr(c, field, (ctypes.c_float * 3)(*[x * scale for x in getattr(c, field)]))
      with pytest.raises(ValueError, match=r'srl_render_camera: fwd and light must be unit vectors \(to 1e-3\)'):
        g._camera_call(c, None, rgb, None, None)
    c = cam.to_c(16, 8)
    setattr(c, 'fwd', (ctypes.c_float * 3)(*[x * 1.0005 for x in c.fwd]))      # within 1e-3: taken
    g._camera_call(c, None, rgb, None, None)
    sc = [torch.as_tensor(a).cuda() for a in cc.pile_scene(ref_pool, 1)]
    for k in range(4):
      part = list(sc)
      part[k] = None
      with pytest.raises(ValueError, match='srl_render_camera: the scene pointers .* must be all set or all NULL'):
        g._camera_call(cam.to_c(16, 8), part, rgb, None, None)
    with pytest.raises(ValueError, match='srl_render_camera: all outputs are NULL'):
      g.render_camera(16, 8, camera=cam, rgb=False, depth=False, ids=False)
    for mode in ('human', 'camera'):                     # `render` keeps the reference's modes
      with pytest.raises(ValueError, match="Only 'rgb_array' is supported"):
        g.render(mode)
    torch.cuda.synchronize()
  finally:
    g.close()


def test_a_view_only_reads_the_env(ref_pool):
  """The state records before and after a view are bit-equal, and the next step's outputs equal those of a twin env that
  never rendered."""
  B = 3
  g, twin = _env(ref_pool, B), _env(ref_pool, B)
  try:
    for e in (g, twin):
      _script(e, ref_pool, 29)
      e.reset()
      e.step(_pixels(e, 0))
    before = g.get_state()
    for name in ('reference', 'closeup', 'noshadow'):
      g.render_camera(64, 48, camera=cc.cameras()[name], rgb=True, depth=True, ids=True)
    g.render_camera(41, 23, scene=cc.grid_scene(ref_pool, B))
    after = g.get_state()
    assert torch.equal(before.records, after.records)
    a, b = g.step(_pixels(g, 1)), twin.step(_pixels(twin, 1))
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
  finally:
    g.close(); twin.close()
