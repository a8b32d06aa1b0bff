"""GPU tests of `render('rgb_array')` (csrc/view.hip behind `srl_render_rgb`): in every state of an episode the images are,
bit for bit, tests/view_cases.py's restatement of the reference's `StackEnv.render` (held to the reference's own images by
tests/test_view.py) applied to exactly the arrays `maps()` returns — float64 like the reference's, and the uint8 frames.

Shapes: the workgroup's 256 threads cover 1,024 pixels a round as float64 (runs of 4) and 4,096 as uint8 (runs of 16).
  128 / 32  the default: 16 / 4 rounds over the overhead map, 1 / a quarter over the object map
  64 / 16   4 / 1 rounds; the object map takes a quarter / a sixteenth of the threads
  96 / 32   9 rounds as float64, 2.25 as uint8: the last round is partial, and a row is no power of two wide
  32 / 8    1 round / a quarter; the object map's 64 pixels are 16 / 4 runs"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import view_cases as vc

pytestmark = pytest.mark.gpu

SHAPES = {'128/32': {}, '64/16': dict(resolution_factor=4), '96/32': dict(observable_size_ratio=3), '32/8': dict(resolution_factor=3)}


def _script(env, pool, seed):
  """Different rocks and a different goal per env: env 0's goal starts in the first row and column, env 1's ends in the last."""
  B, L, H, h = env.batch_size, env.config.episode_length, env.config.overhead_res, env.config.object_res
  rng = np.random.RandomState(seed)
  ids = np.stack([rng.choice(len(pool), size=L, replace=False) for _ in range(B)]).astype(np.int32)
  rect = np.zeros((B, 4), np.int32)
  for i in range(B):
    gh, gw = rng.randint(h, H // 2), rng.randint(h, H // 2 + 1) + 1
    u, v = (0, 0) if i == 0 else (H - gh, H - gw) if i == 1 else (rng.randint(0, H - gh), rng.randint(0, H - gw))
    rect[i] = (u, v, gh, gw)
  env.set_script(ids, rect)
  return rect


def _pixels(env, k):
  """Placements near the centre of the action map, another pixel per env and step."""
  AW = env.config.overhead_res - env.config.object_res + 1
  i = AW // 2 + (np.arange(env.batch_size) * 3 + k * 5) % 7 - 3
  j = AW // 2 - (np.arange(env.batch_size) * 2 + k * 3) % 5 + 2
  return torch.as_tensor(i * AW + j, dtype=torch.int64)


def _same(got, want, tag):
  got = got.cpu().numpy()
  assert got.shape == want.shape and got.dtype == want.dtype, '{}: {} {} for {} {}'.format(tag, got.dtype, got.shape, want.dtype, want.shape)
  if not vc.bits_equal(got, want):
    bad = np.argwhere(got.view(np.uint64 if got.dtype == np.float64 else np.uint8) != want.view(np.uint64 if want.dtype == np.float64 else np.uint8))
    raise AssertionError('{}: {} elements differ, first at {}: {!r} for {!r}'.format(tag, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _check(env, tag):
  """render() in both types against the references of maps(), taken after it."""
  f0, f1 = env.render()
  b0, b1 = env.render('rgb_array', dtype='uint8')
  maps = env.maps()
  assert f0.dtype == torch.float64 and b0.dtype == torch.uint8
  r0, r1 = vc.batch_reference(maps)
  _same(f0, r0, tag + ' rgb0'); _same(f1, r1, tag + ' rgb1')
  u0, u1 = vc.batch_reference(maps, vc.uint8_reference)
  _same(b0, u0, tag + ' rgb0 uint8'); _same(b1, u1, tag + ' rgb1 uint8')
  return maps, (r0, r1)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_render_through_an_episode(ref_pool, shape, B):
  """Before the first reset, after it, after every placement, after the last one (nothing pending) and after the auto-reset."""
  from stackrl_amd import env as envs
  L = 3
  g = envs.VecStackEnv(n_parallel=B, seed=3, pool=ref_pool, block=True, episode_length=L, **SHAPES[shape])
  try:
    maps, _ = _check(g, 'new')                           # all-zero overhead maps: the max == 0 branch
    assert maps[0].max() == 0
    rect = _script(g, ref_pool, 5)
    g.reset()
    maps, _ = _check(g, 'reset')
    assert maps[0].max() == 0 and np.array_equal(maps[2], rect)
    seen = []
    for k in range(L):
      _, _, done = g.step(_pixels(g, k))
      maps, ref = _check(g, 'step {}'.format(k))
      assert (maps[0].reshape(B, -1).max(1) > 0).all()
      seen.append(maps)
    assert bool(done.all())
    H = g.config.overhead_res
    # the cases are what they claim: each env has its own max and goal; the last state has no rock pending (a constant map)
    if B > 1:
      assert len({float(x) for x in maps[0].reshape(B, -1).max(1)}) == B and len({tuple(r) for r in maps[2]}) == B
      assert ref[0][0, 0, 0, 1] == 0.5 + 0.1 and ref[0][1, H - 1, H - 1, 1] == 0.5 + 0.1 and ref[0][1, 0, 0, 1] == 0.5
    assert (maps[1].reshape(B, -1).min(1) == maps[1].reshape(B, -1).max(1)).all()
    assert (seen[0][1].reshape(B, -1).min(1) < seen[0][1].reshape(B, -1).max(1)).all()
    g.step(_pixels(g, 0))                                # env.py:235-236: the auto-reset
    maps, _ = _check(g, 'auto-reset')
    assert maps[0].max() == 0
  finally:
    g.close()


def test_render_with_orientation_freedom(ref_pool):
  """Stack-v2, four orientations: the object view is orientation 0 of the pending rock (`n[0]`, env.py:563)."""
  from stackrl_amd import env as envs
  B, L = 3, 3
  g = envs.make('Stack-v2', n_parallel=B, seed=7, pool=ref_pool, block=True, episode_length=L, orientation_freedom=2)
  try:
    _script(g, ref_pool, 9)
    g.reset()
    maps, _ = _check(g, 'reset')
    assert maps[1].shape == (B, 4, 32, 32) and not np.array_equal(maps[1][:, 0], maps[1][:, 1])
    A = g.config.n_actions
    for k in range(L):
      g.step((k + 1) % 4 * A + _pixels(g, k))
      _check(g, 'step {}'.format(k))
  finally:
    g.close()


def test_render_with_ordering_freedom(ref_pool):
  """Stack-v2 with every rock on show: the object view is the first rock still unplaced, whichever the action took, and the
  empty map after the last."""
  from stackrl_amd import env as envs
  B, L = 3, 3
  g = envs.make('Stack-v2', n_parallel=B, seed=7, pool=ref_pool, block=True, episode_length=L, orientation_freedom=1, ordering_freedom=True)
  try:
    _script(g, ref_pool, 13)
    g.reset()
    maps, _ = _check(g, 'reset')
    assert maps[1].shape == (B, 2 * L, 32, 32)
    first = [maps[1][:, 0].copy()]
    A = g.config.n_actions
    for k, rock in enumerate((1, 0, 0)):                 # the second rock on show first: map 0 stays; then the first: it changes
      g.step((rock * 2 + k % 2) * A + _pixels(g, k))
      maps, _ = _check(g, 'step {} (rock {})'.format(k, rock))
      first.append(maps[1][:, 0].copy())
    assert np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])
    assert (first[3].reshape(B, -1).min(1) == first[3].reshape(B, -1).max(1)).all()      # nothing left on show
  finally:
    g.close()


def test_out_tensors_are_filled_in_place(ref_pool):
  from stackrl_amd import env as envs
  B = 2
  g = envs.VecStackEnv(n_parallel=B, seed=3, pool=ref_pool, block=True, episode_length=2)
  try:
    _script(g, ref_pool, 17)
    g.reset()
    g.step(_pixels(g, 0))
    r0, r1 = vc.batch_reference(g.maps())
    for dtype, ref in ((None, (r0, r1)), ('uint8', vc.batch_reference(g.maps(), vc.uint8_reference))):
      dt = torch.float64 if dtype is None else torch.uint8
      # views of a larger batch, as `PipelinedVecStackEnv.render` passes them
      big0 = torch.full((B + 2, 128, 128, 3), 7, dtype=dt, device='cuda')
      big1 = torch.full((B + 2, 32, 32, 3), 7, dtype=dt, device='cuda')
      out = (big0[1:1 + B], big1[1:1 + B])
      got = g.render(dtype=dtype, out=out)
      assert got[0] is out[0] and got[1] is out[1]
      _same(big0[1:1 + B], ref[0], 'out rgb0'); _same(big1[1:1 + B], ref[1], 'out rgb1')
      assert bool((big0[0] == 7).all() and (big0[-1] == 7).all() and (big1[0] == 7).all() and (big1[-1] == 7).all())
      # images that start one element into a 16-byte line: no 128-bit stores, the pixel-by-pixel path, nothing beyond the ends
      n0, n1 = B * 128 * 128 * 3, B * 32 * 32 * 3
      flat0 = torch.full((n0 + 2,), 7, dtype=dt, device='cuda')
      flat1 = torch.full((n1 + 2,), 7, dtype=dt, device='cuda')
      assert flat0.data_ptr() % 16 == 0 and flat1.data_ptr() % 16 == 0
      out = (flat0[1:1 + n0].view(B, 128, 128, 3), flat1[1:1 + n1].view(B, 32, 32, 3))
      g.render(dtype=dtype, out=out)
      _same(out[0], ref[0], 'unaligned rgb0'); _same(out[1], ref[1], 'unaligned rgb1')
      assert bool(flat0[0] == 7) and bool(flat0[-1] == 7) and bool(flat1[0] == 7) and bool(flat1[-1] == 7)
    with pytest.raises(ValueError, match='out must be'):
      g.render(out=(torch.empty((B, 128, 128, 3), dtype=torch.float32, device='cuda'), torch.empty((B, 32, 32, 3), dtype=torch.float64, device='cuda')))
  finally:
    g.close()


def test_render_after_a_step_that_was_not_waited_for(ref_pool):
  """side_stream: `render()` right after a non-blocking `step` is ordered after that step's kernels and shows its maps."""
  from stackrl_amd import env as envs
  B = 3
  g = envs.VecStackEnv(n_parallel=B, seed=3, pool=ref_pool, block=False, episode_length=3, side_stream=True)
  try:
    _script(g, ref_pool, 19)
    g.reset()()
    before = g.render()[0].clone()
    wait = g.step(_pixels(g, 0))
    f0, f1 = g.render()                                  # the step has not been waited for
    wait()
    r0, r1 = vc.batch_reference(g.maps())
    _same(f0, r0, 'rgb0'); _same(f1, r1, 'rgb1')
    assert not torch.equal(before, f0)
  finally:
    g.close()


def test_pipelined_render_is_its_groups_in_env_order(ref_pool):
  from stackrl_amd import env as envs
  B = 4
  g = envs.PipelinedVecStackEnv(n_parallel=B, groups=2, seed=3, pool=ref_pool, block=True, episode_length=3)
  try:
    _script(g, ref_pool, 23)
    g.reset()
    g.step(_pixels(g, 0))
    for dtype in (None, 'uint8'):
      got = g.render(dtype=dtype)
      parts = [e.render(dtype=dtype) for e in g._envs]
      for k in range(2):
        assert torch.equal(got[k], torch.cat([p[k] for p in parts]))
    _check(g, 'pipelined')
    with pytest.raises(ValueError, match="'rgb_array'"):
      g.render('human')
  finally:
    g.close()


def test_started_env_inherits_render(ref_pool):
  from stackrl_amd import env as envs
  g = envs.make('Stack-v1', n_parallel=2, seed=3, pool=ref_pool, block=True, episode_length=2, n_objects=4)
  try:
    g.reset()                                            # two rocks placed by the start policy
    maps, _ = _check(g, 'started')
    assert (maps[0].reshape(2, -1).max(1) > 0).all()
  finally:
    g.close()


def test_bad_arguments_are_refused(ref_pool):
  from stackrl_amd import env as envs
  g = envs.VecStackEnv(n_parallel=1, seed=3, pool=ref_pool, block=True, episode_length=2)
  try:
    for mode in ('human', 'rgb', None):
      with pytest.raises(ValueError, match="Only 'rgb_array' is supported"):
        g.render(mode)
    for dtype in ('float32', torch.float16, 'colour'):
      with pytest.raises(ValueError, match=r'srl_render_rgb: dtype must be 0 \(float64\) or 1 \(uint8\)'):
        g.render(dtype=dtype)
    assert g.render(dtype=np.uint8)[0].dtype == torch.uint8 and g.render(dtype=torch.float64)[0].dtype == torch.float64
  finally:
    g.close()
