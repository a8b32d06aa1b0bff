"""libstackrl_rocks.so on the device (include/stackrl_rocks.h; csrc/rocks.hip) against the numpy restatement of
tests/rocks_cases.py, against float64 recomputations from its own outputs, against the host generator's pool, and through
`VecStackEnv.set_pool` against the oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch

import rocks_cases as rc
from stackrl_amd import assets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS = 0.0625
FIELDS = ('verts', 'vert_src', 'tris', 'counts', 'mass_com', 'inertia', 'xform', 'metrics', 'status')
N, IRR, SEED = 67, 0.5, 11


def _rocks():
  from stackrl_amd import rocks
  return rocks


def _np(b):
  return {k: getattr(b, k).cpu().numpy() for k in FIELDS}


def _same(a, b, rows=slice(None), rows_b=None):
  a, b = _np(a), _np(b)
  for k in FIELDS:
    assert np.array_equal(a[k][rows].view(np.uint32), b[k][rows if rows_b is None else rows_b].view(np.uint32)), k


@pytest.fixture(scope='module')
def batch():
  """67 rocks (more than one wave's worth of workgroups, an odd count) with their points, read back once."""
  b = _rocks().generate(N, IRR, seed=SEED, return_points=True)
  out = _np(b)
  out['points'] = b.points.cpu().numpy()
  out['batch'] = b
  return out


@pytest.fixture(scope='module')
def pool500():
  return _rocks().generate_pool(500, seed=11)


def _ulps(got, ref):
  return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('subdivisions', [0, 1, 3])
def test_points_are_the_restatements_also_past_index_2_32(n, subdivisions):
  """Within 2 float32 ulps of the value: the device's normcdfinv and scipy's ndtri differ in the last bits of a float64,
  which moves a point by one float32 ulp where it straddles a rounding boundary."""
  first = 2 ** 32 - 1                    # rock 1 of the batch has a non-zero high counter word
  for irr in (0.05, 0.95):
    b = _rocks().generate(n, irr, seed=3, first_index=first, subdivisions=subdivisions, return_points=True)
    got = b.points.cpu().numpy()
    assert got.shape == (n, rc.POINTS[subdivisions], 3)
    worst = 0.0
    for i in range(n):
      ref = rc.points(first + i, irregularity=irr, subdivisions=subdivisions, seed=3)
      worst = max(worst, float(_ulps(got[i], ref).max()))
    print('subdivisions {} irregularity {}: {} ulps'.format(subdivisions, irr, worst))
    assert worst <= 2.0
    assert (b.status.cpu().numpy() == 0).all()
    # the low word alone does not name the rock
    low = _rocks().generate(1, irr, seed=3, first_index=0, subdivisions=subdivisions, return_points=True).points.cpu().numpy()
    assert n < 2 or not np.array_equal(low[0], got[1])


def test_two_calls_and_the_points_fed_back_give_the_same_bits(batch):
  rocks = _rocks()
  again = rocks.generate(N, IRR, seed=SEED, return_points=True)
  _same(batch['batch'], again)
  assert torch.equal(again.points, batch['batch'].points)
  fed = rocks.generate(N, IRR, seed=SEED, points=batch['batch'].points)
  _same(batch['batch'], fed)


def test_a_rock_does_not_depend_on_its_batch(batch):
  rocks = _rocks()
  for i in (0, 1, 40, 66):
    _same(batch['batch'], rocks.generate(1, IRR, seed=SEED, first_index=i), rows=slice(i, i + 1), rows_b=slice(0, 1))
  _same(batch['batch'], rocks.generate(2, IRR, seed=SEED, first_index=64), rows=slice(64, 66), rows_b=slice(0, 2))


def test_vertices_are_the_transform_of_their_source_points(batch):
  assert (batch['status'] == 0).all()
  bound = 16 * float(np.spacing(np.float32(0.125)))              # a scale, a 3-term dot product and a subtraction in float32
  worst = worst_r = 0.0
  for i in range(N):
    nv, nt = batch['counts'][i]
    src = batch['vert_src'][i, :nv]
    assert (np.diff(src) > 0).all() and (batch['vert_src'][i, nv:] == -1).all() and src.min() >= 0 and src.max() < 386
    ref = rc.apply_xform(batch['xform'][i], batch['points'][i][src])
    worst = max(worst, float(np.abs(batch['verts'][i, :nv] - ref).max()))
    R = batch['xform'][i, 1:10].reshape(3, 3).astype(np.float64)
    worst_r = max(worst_r, float(np.abs(R @ R.T - np.eye(3)).max()), abs(float(np.linalg.det(R)) - 1.0))
    assert (batch['verts'][i, nv:] == 0).all() and (batch['tris'][i, nt:] == 0).all()
    assert 0 < batch['xform'][i, 0] <= 1
  print('vertex error {} (bound {}), rotation error {}'.format(worst, bound, worst_r))
  assert worst <= bound and worst_r <= 1e-6


def test_the_vertex_set_is_the_restatements(batch):
  """The cap of the issue: rocks with any difference number <= 2 %, each differing point within 1e-6 radius of a face plane
  of the other hull.  (On these seeds the device and the restatement agree on every rock.)"""
  differing = 0
  for i in range(24):
    nv, nt = batch['counts'][i]
    status, src, tris = rc.hull(batch['points'][i])
    assert status == 0
    got = batch['vert_src'][i, :nv]
    if not np.array_equal(got, src):
      differing += 1
      hp = batch['points'][i].astype(np.float64)
      for k in set(got) - set(src):                     # the device's, not the restatement's: on a face plane of the restatement's hull
        assert abs(rc.max_outside(hp[src], tris, hp[[k]])) <= 1e-6 * RADIUS
      for k in set(src) - set(got):                     # the restatement's, not the device's: on a face plane of the device's hull
        assert abs(rc.max_outside(hp[got], batch['tris'][i, :nt], hp[[k]])) <= 1e-6 * RADIUS
    else:
      assert np.array_equal(batch['tris'][i, :nt], tris)       # the same wrap: the same triangles in the same order
  assert differing <= 0.02 * 24


def test_the_mesh_is_closed_outward_and_holds_every_point(batch):
  worst = -np.inf
  for i in range(N):
    nv, nt = batch['counts'][i]
    v, t = batch['verts'][i, :nv], batch['tris'][i, :nt]
    assert 4 <= nv <= 128 and nt == 2 * nv - 4 and t.min() >= 0 and t.max() < nv
    assert rc.closed_outward(v, t)
    worst = max(worst, rc.max_outside(v, t, rc.apply_xform(batch['xform'][i], batch['points'][i])))
  print('furthest point in front of a face: {} (bound {})'.format(worst, 1e-6 * RADIUS))
  assert worst <= 1e-6 * RADIUS


def test_mass_inertia_and_metrics_are_those_of_the_returned_vertices(batch):
  worst = {'volume': 0.0, 'com': 0.0, 'inertia': 0.0, 'metrics': 0.0}
  for i in range(N):
    nv, nt = batch['counts'][i]
    v, t = batch['verts'][i, :nv], batch['tris'][i, :nt]
    rho = rc.density(i, SEED)
    volume, com, inertia = rc.mass_inertia(v, t, rho)
    fe = v.astype(np.float64).max(0) - v.astype(np.float64).min(0)
    metrics = np.array([volume, volume / fe.prod(), fe.max() / fe.min(), fe.prod()])
    rel = lambda got, ref: float(np.abs((got.astype(np.float64) - ref) / ref).max())
    worst['volume'] = max(worst['volume'], rel(batch['mass_com'][i, :1], np.array([rho * volume])))
    worst['com'] = max(worst['com'], float(np.abs(batch['mass_com'][i, 1:] - com).max()))
    worst['inertia'] = max(worst['inertia'], rel(batch['inertia'][i], inertia))
    worst['metrics'] = max(worst['metrics'], rel(batch['metrics'][i], metrics))
    assert fe[0] >= fe[1] >= fe[2]                               # final extents x >= y >= z
    assert 2200 <= rho <= 2600
  print(worst)
  assert worst['volume'] <= 1e-6 and worst['inertia'] <= 1e-6 and worst['metrics'] <= 1e-6 and worst['com'] <= 1e-7


def test_the_box_is_the_host_searchs_within_1e_5(batch):
  worst = 0.0
  for i in range(8):
    nv, nt = batch['counts'][i]
    v, t = batch['verts'][i, :nv].astype(np.float64), batch['tris'][i, :nt]
    _, _, ext = assets.oriented_bounds(v, t)
    worst = max(worst, abs(float(batch['metrics'][i, 3]) / ext.prod() - 1.0))
  print('box volume against assets.oriented_bounds: {}'.format(worst))
  assert worst <= 1e-5


def test_fit_1_scales_to_the_longest_box_extent():
  b = _rocks().generate(5, 0.95, seed=5, fit=1)
  v, c = b.verts.cpu().numpy(), b.counts.cpu().numpy()
  for i in range(5):
    ext = v[i, :c[i, 0]].max(0) - v[i, :c[i, 0]].min(0)
    assert ext[0] <= 2 * RADIUS * (1 + 1e-6) and ext[0] >= ext[1] >= ext[2]
    assert abs(ext[0] - 2 * RADIUS) <= 1e-6 * RADIUS or float(b.xform[i, 0]) == 1.0


def test_a_tetrahedron_given_as_points():
  b = _rocks().generate(1, points=torch.from_numpy(rc.tetrahedron()[None]).cuda())
  o = _np(b)
  assert o['status'][0] == 0 and tuple(o['counts'][0]) == (4, 4) and list(o['vert_src'][0, :4]) == [0, 1, 2, 3]
  assert rc.closed_outward(o['verts'][0, :4], o['tris'][0, :4])
  ref = rc.rock(pts=rc.tetrahedron())
  assert np.array_equal(o['tris'][0, :4], ref['tris'])
  assert np.abs(o['verts'][0, :4] - ref['verts']).max() <= 16 * float(np.spacing(np.float32(0.125)))


# ------------------------------------------------------------------------------------------------ edge cases behind sentinels
SENTINEL = 0x5e471e1
_SHAPES = (('verts', (128, 3), torch.float32), ('vert_src', (128,), torch.int32), ('tris', (252, 3), torch.int32),
           ('counts', (2,), torch.int32), ('mass_com', (4,), torch.float32), ('inertia', (6,), torch.float32),
           ('xform', (13,), torch.float32), ('metrics', (4,), torch.float32), ('status', (), torch.int32))


def _raw(points):
  """`srl_rocks_generate` on given points with every output buffer followed by 64 sentinel words; returns the outputs (numpy)
  after checking the sentinels."""
  rocks = _rocks()
  n, P = points.shape[:2]
  pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).cuda()
  bufs, views = {}, {}
  for name, shape, dt in _SHAPES + (('points_out', (P, 3), torch.float32),):
    words = n * int(np.prod(shape, dtype=np.int64))
    bufs[name] = torch.full((words + 64,), SENTINEL, dtype=torch.int32, device='cuda')
    views[name] = bufs[name][:words].view(dt).reshape((n,) + shape)
  par = rocks.Params(RADIUS, 0.5, (ctypes.c_float * 3)(1.0, 0.5, 1 / 3), 3, 2200.0, 2600.0, 0, 11)
  rocks.call('srl_rocks_generate', pts, ctypes.byref(par), 0, n, pts, P, views['points_out'],
             *[views[name] for name, _, _ in _SHAPES])
  torch.cuda.synchronize()
  for name, b in bufs.items():
    assert (b[-64:] == SENTINEL).all(), name
  return {k: v.cpu().numpy() for k, v in views.items()}


def test_overflow_is_reported_for_that_rock_only():
  sphere = rc.sphere_points(200)
  assert rc.hull(sphere)[0] == rc.OVERFLOW                       # the restatement first: the same loop bounds
  good = rc.points(0)[:200]
  assert rc.hull(good)[0] == rc.OK
  o = _raw(np.stack([good, sphere, rc.points(1)[:200]]))
  assert list(o['status']) == [0, 1, 0]
  assert tuple(o['counts'][1]) == (0, 0) and (o['verts'][1] == 0).all() and (o['vert_src'][1] == -1).all()
  assert np.array_equal(o['points_out'][1], sphere)
  for i in (0, 2):
    nv, nt = o['counts'][i]
    assert rc.closed_outward(o['verts'][i, :nv], o['tris'][i, :nt])
    assert np.array_equal(o['vert_src'][i, :nv], rc.hull(o['points_out'][i])[1])


def test_exactly_coplanar_points_end_in_status_2_or_the_hull_of_the_corners():
  box = rc.coplanar_box(2)
  status = rc.hull(box)[0]                                        # the restatement first
  assert status in (rc.OK, rc.DEGENERATE)
  o = _raw(np.stack([box, rc.points(0, subdivisions=2)]))
  assert o['status'][1] == 0
  assert o['status'][0] in (0, 2)
  if o['status'][0] == 0:
    nv, nt = o['counts'][0]
    assert sorted(o['vert_src'][0, :nv]) == list(range(8)) and rc.closed_outward(o['verts'][0, :nv], o['tris'][0, :nt])
  else:
    assert tuple(o['counts'][0]) == (0, 0)


def test_near_coplanar_points_close_on_the_restatements_vertex_set():
  """Points coplanar to within an ulp or so: the float64 predicate decides them as the restatement does (a float32 one ends
  in status 2 on every one of these, tests/test_rocks_cases.py)."""
  pts = np.stack([rc.near_coplanar(k) for k in range(8)])
  o = _raw(pts)
  assert (o['status'] == 0).all()
  for k in range(8):
    status, src, tris = rc.hull(pts[k])
    nv, nt = o['counts'][k]
    assert status == 0 and np.array_equal(o['vert_src'][k, :nv], src) and np.array_equal(o['tris'][k, :nt], tris)


# ------------------------------------------------------------------------------------------------ pools and the env
def _pool_statistics(pool):
  ext, nv, vol = [], [], []
  for i in range(len(pool)):
    v, t, _ = pool.mesh(i)
    v = v.astype(np.float64)
    ext.append(np.sort(v.max(0) - v.min(0)))
    nv.append(len(v))
    vol.append(assets.mass_properties(v, t)[0])
  ext = np.array(ext)
  return {'extent0': ext[:, 0], 'extent1': ext[:, 1], 'extent2': ext[:, 2], 'vertices': np.array(nv, dtype=np.float64), 'volume': np.array(vol)}


def test_a_pool_of_500_has_the_statistics_of_the_shipped_pool(pool500):
  assert len(pool500) == 500 and pool500.names[0] == '50_000' and pool500.names[-1] == '95_049'
  host = assets.default_pool()
  d, h = _pool_statistics(pool500), _pool_statistics(host)
  for k in d:
    bound = 4 * np.sqrt(d[k].var(ddof=1) / len(d[k]) + h[k].var(ddof=1) / len(h[k]))
    print('{}: device {} host {} bound {}'.format(k, d[k].mean(), h[k].mean(), bound))
    assert abs(d[k].mean() - h[k].mean()) <= bound, k


def test_set_pool_resets_and_steps_with_the_oracle(pool500):
  from oracle.oracle import OracleEnv
  from stackrl_amd import env as envs
  from stackrl_amd.config import StackConfig
  first = assets.MeshPool.load(os.path.join(ROOT, 'tests', 'golden', 'ref_rocks.npz'))
  n, L = 8, 4
  g = envs.VecStackEnv(n_parallel=n, seed=11, pool=first, block=True, episode_length=L, device='cuda:0')
  try:
    g.reset()
    g.step(g.sample())
    before = g.state_signature()
    g.set_pool(pool500)
    assert g.state_signature() != before and g.pool is pool500
    with pytest.raises(RuntimeError, match='needs a reset first'):
      g.step(g.sample())
    g.seed(11)
    o = OracleEnv(StackConfig(n_envs=n, episode_length=L), pool500, seed=11)
    (gm, go), _, _ = g.reset()
    (om, oo), _, _ = o.reset()
    assert np.array_equal(gm.cpu().numpy(), om) and np.array_equal(go.cpu().numpy(), oo)
    for _ in range(L + 1):
      a = g.sample()
      (gm, go), gr, gd = g.step(a)
      (om, oo), orr, od = o.step(a.cpu().numpy())
      assert np.array_equal(gm.cpu().numpy(), om) and np.array_equal(go.cpu().numpy(), oo)
      assert np.array_equal(gd.cpu().numpy(), od) and np.array_equal(gr.cpu().numpy(), orr)
  finally:
    g.close()


def test_set_pool_reaches_every_group_of_the_pipelined_env(pool500):
  from stackrl_amd import env as envs
  first = assets.MeshPool.load(os.path.join(ROOT, 'tests', 'golden', 'ref_rocks.npz'))
  n, L = 8, 4
  p = envs.PipelinedVecStackEnv(n_parallel=n, groups=2, seed=11, pool=first, block=True, episode_length=L)
  g = envs.VecStackEnv(n_parallel=n, seed=11, pool=pool500, block=True, episode_length=L)
  try:
    p.reset()
    p.step(p.sample())
    p.set_pool(pool500)
    assert p.pool is pool500 and p.state_signature() == g.state_signature()
    with pytest.raises(RuntimeError, match='needs a reset first'):
      p.step(torch.zeros(n, dtype=torch.int64))
    p.seed(11)
    (pm, po), _, _ = p.reset()
    (gm, go), _, _ = g.reset()
    assert torch.equal(pm, gm) and torch.equal(po, go)
    a = g.sample()
    (pm, po), pr, pd = p.step(a)
    (gm, go), gr, gd = g.step(a)
    assert torch.equal(pm, gm) and torch.equal(po, go) and torch.equal(pr, gr) and torch.equal(pd, gd)
    g.set_script(np.zeros((n, L), dtype=np.int32), np.tile(np.array([[40, 40, 48, 48]], dtype=np.int32), (n, 1)))
    with pytest.raises(RuntimeError, match='set_script after set_pool'):
      g.set_pool(first)
  finally:
    p.close()
    g.close()


def test_a_lookahead_follows_set_pool(pool500):
  """The scratch env of a `Lookahead` made before `set_pool` loads the new pool at the next `evaluate` (the new pool is the
  larger one: its mesh ids do not exist in the old table), and `evaluate` is refused while the env itself waits for its reset."""
  from stackrl_amd import env as envs
  from stackrl_amd.lookahead import Lookahead
  first = assets.MeshPool.load(os.path.join(ROOT, 'tests', 'golden', 'ref_rocks.npz'))
  n, L = 4, 4
  g = envs.VecStackEnv(n_parallel=n, seed=11, pool=first, block=True, episode_length=L)
  look = Lookahead(g, 2)
  fresh = None
  try:
    g.reset()
    look.evaluate(torch.stack([g.sample(), g.sample()], dim=1))
    g.set_pool(pool500)
    with pytest.raises(RuntimeError, match='needs a reset first'):
      look.evaluate(torch.zeros((n, 2), dtype=torch.int64))
    g.seed(11)
    g.reset()
    actions = torch.stack([g.sample(), g.sample()], dim=1)
    r, d = look.evaluate(actions)
    assert look.scratch.pool is pool500 and look.signature == g.state_signature()
    fresh = Lookahead(g, 2)
    r2, d2 = fresh.evaluate(actions)
    assert torch.equal(r, r2) and torch.equal(d, d2)
    _, gr, gd = g.step(actions[:, 0])
    assert torch.equal(gr, r[:, 0]) and torch.equal(gd, d[:, 0])
  finally:
    look.close()
    if fresh is not None:
      fresh.close()
    g.close()


def test_what_lifts_and_what_keeps_the_refusals_of_set_pool(pool500):
  from stackrl_amd import env as envs
  first = assets.MeshPool.load(os.path.join(ROOT, 'tests', 'golden', 'ref_rocks.npz'))
  n, L = 4, 4
  g = envs.VecStackEnv(n_parallel=n, seed=11, pool=first, block=True, episode_length=L)
  h = envs.VecStackEnv(n_parallel=n, seed=11, pool=pool500, block=True, episode_length=L)
  s = envs.StartedVecStackEnv(n_parallel=n, seed=11, pool=first, block=True, episode_length=2, n_objects=3)
  try:
    # a whole-batch set_state of a state of the new table stands for the reset
    g.reset()
    h.reset()
    h.step(h.sample())
    g.set_pool(pool500)
    g.set_state(h.get_state())
    a = h.sample()
    (gm, go), gr, gd = g.step(a)
    (hm, ho), hr, hd = h.step(a)
    assert torch.equal(gm, hm) and torch.equal(go, ho) and torch.equal(gr, hr) and torch.equal(gd, hd)
    # a script is taken by the auto-reset inside step as by reset: set_pool is free again after it
    h.reset()
    h.set_script(np.zeros((n, L), dtype=np.int32), np.tile(np.array([[40, 40, 48, 48]], dtype=np.int32), (n, 1)))
    with pytest.raises(RuntimeError, match='set_script after set_pool'):
      h.set_pool(first)
    for _ in range(L + 1):
      h.step(h.sample())
    h.set_pool(first)
    # a refused step of the started env does not count
    s.reset()
    before = s._since_reset
    s.set_pool(pool500)
    with pytest.raises(RuntimeError, match='needs a reset first'):
      s.step(torch.zeros(n, dtype=torch.int64))
    assert s._since_reset == before
    s.reset()
    s.step(s.sample())
  finally:
    g.close()
    h.close()
    s.close()
