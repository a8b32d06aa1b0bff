"""GPU tests of the env library's host side (csrc/stackrl_hip.hip) and of `VecStackEnv._launch`: a refused `set_pool` leaves the
live env exactly as it was, and `render_heightmap` on a side stream waits for its inputs and is waited for.  Every comparison
is exact, run against run."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pool():
  from stackrl_amd import assets
  return assets.default_pool()


def _open_tetrahedron():
  """A regular tetrahedron that has lost a face.  Three triangles are refused by the count check before the surface is looked
  at, so the face (1, 3, 2) is split at its centroid first (a closed surface of 5 vertices and 6 triangles, the smallest the
  count check admits beside the plain one) and the face (0, 1, 2) is the one removed."""
  from stackrl_amd import assets
  v = 0.03125 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
  v = np.concatenate([v, v[[1, 3, 2]].mean(0, keepdims=True)]).astype(np.float32)
  t = np.array([[0, 2, 3], [0, 3, 1], [1, 3, 4], [3, 2, 4], [2, 1, 4]], np.int32)
  return assets.pack([(v, t, np.array([1.5, 0, 0, 0], np.float32))], ['open_tetrahedron'])


def _same(a, b, tag):
  (am, ao), ar, ad = a
  (bm, bo), br, bd = b
  assert torch.equal(am, bm) and torch.equal(ao, bo), tag + ': observations differ'
  assert torch.equal(ar.view(torch.int32), br.view(torch.int32)), tag + ': rewards differ'
  assert torch.equal(ad, bd), tag + ': dones differ'


def _same_state(a, b, tag):
  for x, y in zip(a.state(), b.state()):
    assert np.array_equal(x.view(np.int32), y.view(np.int32)), tag + ': state() differs'


def test_a_refused_set_pool_leaves_the_live_env_as_it_was(pool):
  from stackrl_amd import env as envs
  a, b = (envs.VecStackEnv(n_parallel=2, episode_length=2, seed=7, pool=pool, block=True) for _ in range(2))
  _same(a.reset(), b.reset(), 'reset')
  rng = np.random.RandomState(3)
  acts = torch.from_numpy(rng.randint(0, a.n_actions, size=(4, 2)).astype(np.int64)).cuda()
  _same(a.step(acts[0]), b.step(acts[0]), 'step 0')
  with pytest.raises(ValueError) as e:
    a.set_pool(_open_tetrahedron())
  assert str(e.value) == 'mesh is not a closed surface (an edge has only one face)'
  assert a.pool is pool
  _same_state(a, b, 'after the refusal')
  for k in (1, 2, 3):        # the end of the episode, the auto-reset, one step of the next episode
    out = a.step(acts[k])
    _same(out, b.step(acts[k]), 'step {}'.format(k))
    _same_state(a, b, 'step {}'.format(k))
    assert bool(out[2].all()) == (k == 1)
  a.set_pool(pool)
  a.reset()
  a.step(acts[0])
  assert a.state()[1].tolist() == [1, 1]
  a.close(), b.close()


def test_render_heightmap_on_a_side_stream_is_that_of_the_plain_env(pool):
  from stackrl_amd import env as envs
  plain = envs.VecStackEnv(n_parallel=2, episode_length=2, seed=7, pool=pool, block=True)
  side = envs.VecStackEnv(n_parallel=2, episode_length=2, seed=7, pool=pool, block=True, side_stream=True)
  act = torch.tensor([plain.n_actions // 2, plain.n_actions // 3], dtype=torch.int64).cuda()
  plain.reset(), side.reset()
  _same(plain.step(act), side.step(act), 'step')
  poses, nb, _, _ = plain.state()
  assert nb.tolist() == [1, 1]
  maps = []
  for e in (plain, side):
    # the inputs are made on the caller's stream just before the call: the side stream has to wait for them
    p = torch.from_numpy(np.ascontiguousarray(poses[:, :, :7])).cuda()
    ids = torch.from_numpy(np.ascontiguousarray(poses[:, :, 7]).astype(np.int32)).cuda()
    n = torch.from_numpy(nb.astype(np.int32)).cuda()
    maps.append(e.render_heightmap(p, ids, n))
  assert torch.equal(maps[0].view(torch.int32), maps[1].view(torch.int32))
  assert float(maps[0].max()) > float(maps[0].min())          # a rock is on the map
  plain.close(), side.close()
