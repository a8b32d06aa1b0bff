"""Heuristic baseline policies: oracle vs the reference's own golden vectors on CPU,
HIP kernels vs both on the GPU.

Tolerances: `height` is a maximum of exact sums (bit-exact); masks and actions are integers (exact); the float64 sums
of `difference` and `correlate` are taken in another order than numpy's (1e-12 of the largest reference value of the
case); `corrcoef` lies in [-1, 1] and on flat windows is rounding noise of about 1e-16 over rounding noise on both sides
(1e-12 of max(1, largest reference value)); the rows of `difference` whose exponents go through `pow` on the device and
through numpy's `**` on the host, neither correctly rounded, get POW_RTOL."""
import importlib.util
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'baselines_golden.npz')
EDGES = os.path.join(HERE, 'golden', 'baselines_edges_golden.npz')
CASES = [('height', 'height', {}), ('difference', 'difference', {}),
         ('difference_e1w0', 'difference', dict(difference_exponent=1, weights_exponent=0)),
         ('corrcoef', 'corrcoef', {}), ('corrcoef_localized', 'corrcoef', dict(localized=True)),
         ('correlate', 'correlate', {})]
POW_CASES = [('difference_e{}w{}'.format(e, w), 'difference', dict(difference_exponent=e, weights_exponent=w))
             for e, w in ((3, 1), (1, 3), (2, 4))]
THRESHOLDS = (1.0, 0.75, 0.5, 0.0)
SELECT_METHODS = ('height', 'difference', 'corrcoef', 'correlate')
# Largest deviation of a `pow` row from the reference, relative to the largest value of its map, measured on an MI355X:
# 9.6e-16 against the edge golden; 9.8e-16, 4.3e-16 and 2.1e-15 against the oracle on the randomised 64/16, 32/8 and
# 128/32 batches below.  Asserted at five times the largest of them (the issue's ceiling for this figure was 1e-9).
POW_RTOL = 1e-14


@pytest.fixture(scope='module')
def gold():
  return np.load(GOLD)


@pytest.fixture(scope='module')
def edges():
  return np.load(EDGES)


def _make_obs():
  """`make_obs` of the golden generator (seeded blobs, a goal rectangle, a rock-shaped object), loaded by path."""
  spec = importlib.util.spec_from_file_location('make_baselines_golden', os.path.join(HERE, 'golden', 'make_baselines_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod.make_obs


def _uses_pow(fn, kw):
  return fn == 'difference' and (kw.get('difference_exponent', 2) not in (1, 2) or kw.get('weights_exponent', 2) not in (0, 2))


def _bound(fn, kw, ref):
  if fn == 'height':
    return 0.0
  if fn == 'corrcoef':
    return 1e-12 * max(1.0, np.abs(ref).max())
  return (POW_RTOL if _uses_pow(fn, kw) else 1e-12) * max(1e-300, np.abs(ref).max())


def _check_values(fn, kw, got, ref, what, pow_dev=None):
  assert got.shape == ref.shape and np.all(np.isfinite(ref)), what
  err = np.abs(got - ref).max()
  if pow_dev is not None and _uses_pow(fn, kw) and np.abs(ref).max() > 0:
    pow_dev.append(err / np.abs(ref).max())
  assert err <= _bound(fn, kw, ref), (what, err, np.abs(ref).max())


def _groups(edges):
  """The observations of the edge fixture by shape: {(H, h): [names]}, each with its own goal maximum."""
  out = {}
  for n in edges['names']:
    out.setdefault((edges[n + '/map'].shape[0], edges[n + '/obj'].shape[0]), []).append(str(n))
  for (H, h), names in out.items():
    gmax = [int(edges[n + '/map'][:, :, 1].max()) for n in names]
    assert len(names) > 1 and len(set(gmax)) == len(gmax), (H, h, gmax)
  return out


def test_oracle_matches_reference_golden(gold):
  from oracle import baselines_oracle as B
  for k in range(gold['obs_map'].shape[0]):
    inp = (gold['obs_map'][k], gold['obs_obj'][k])
    for name, fn, kw in CASES:
      got = B.METHODS[fn](inp, **kw)
      assert np.abs(got - gold[name][k]).max() <= 1e-12 * max(1e-300, np.abs(gold[name][k]).max()), (name, k)
    assert np.array_equal(B.goal_overlap(inp), gold['goal_overlap'][k])
    for method in ('height', 'difference', 'corrcoef', 'correlate'):
      for goal, mo in ((True, 1), (True, 0), (False, 1)):
        tag = 'select_{}_g{}_m{}'.format(method, int(goal), mo)
        a, v = B.select(gold[method][k], gold['goal_overlap'][k], goal, mo)
        assert a == gold[tag + '_action'][k], (tag, k)
        assert np.allclose(v, gold[tag + '_values'][k], rtol=1e-12, atol=0)


def test_oracle_matches_reference_edges_golden(edges):
  from oracle import baselines_oracle as B
  assert sorted(_groups(edges)) == [(16, 16), (32, 8), (33, 32), (40, 32), (48, 16), (64, 16)]
  for n in edges['names']:
    inp = (edges[n + '/map'], edges[n + '/obj'])
    for name, fn, kw in CASES + POW_CASES:
      got, ref = B.METHODS[fn](inp, **kw), edges[n + '/' + name]
      assert np.abs(got - ref).max() <= 1e-12 * max(1e-300, np.abs(ref).max()), (n, name)
    for t in THRESHOLDS:
      assert np.array_equal(B.goal_overlap(inp, threshold=t), edges['{}/goal_overlap_t{:03d}'.format(n, int(100 * t))]), (n, t)
    mask = edges[n + '/goal_overlap_t100']
    for method in SELECT_METHODS:
      for mo in (0, 1, 2, 3):
        a, v = B.select(edges[n + '/' + method], mask, True, mo)
        assert a == edges['{}/select_{}_g1_m{}_action'.format(n, method, mo)], (n, method, mo)
        assert np.allclose(v, edges['{}/select_{}_g1_values'.format(n, method)], rtol=1e-12, atol=0)
        a, v = B.select(edges[n + '/' + method], None, False, mo)
        assert a == edges['{}/select_{}_g0_m{}_action'.format(n, method, mo)], (n, method, mo)
        assert np.array_equal(v, -edges[n + '/' + method])


@pytest.mark.gpu
def test_hip_value_maps_match_reference(gold):
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  inp = (torch.from_numpy(gold['obs_map']).cuda(), torch.from_numpy(gold['obs_obj']).cuda())
  for name, fn, kw in CASES:
    vals, mask = Bd.heuristic_values(fn, inp, **kw)
    ref = gold[name]
    if fn == 'height':
      assert np.array_equal(vals.cpu().numpy(), ref)                       # max of exact sums: bit-exact
    else:                                                                 # float64 sums in a different order: 1e-12
      assert np.abs(vals.cpu().numpy() - ref).max() <= 1e-12 * max(1e-300, np.abs(ref).max()), name
    assert np.array_equal(mask.cpu().numpy(), gold['goal_overlap'])       # integer arithmetic: exact


@pytest.mark.gpu
def test_hip_selection_matches_reference(gold):
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  mask = torch.from_numpy(gold['goal_overlap']).cuda()
  for method in ('height', 'difference', 'corrcoef', 'correlate'):
    vals = torch.from_numpy(gold[method]).cuda()
    for goal, mo in ((True, 1), (True, 0), (False, 1)):
      tag = 'select_{}_g{}_m{}'.format(method, int(goal), mo)
      a, neg = Bd.select(vals, mask, goal=goal, minorder=mo, value=True)
      assert np.array_equal(a.cpu().numpy(), gold[tag + '_action']), tag   # placement indices bit-exact
      assert np.array_equal(neg.cpu().numpy(), gold[tag + '_values']), tag


@pytest.mark.gpu
def test_baseline_policy_end_to_end(gold, ref_pool):
  """The policy object on live env observations agrees with the oracle on the same observations."""
  torch = pytest.importorskip('torch')
  from oracle import baselines_oracle as B
  from stackrl_amd import baselines as Bd, env as envs
  env = envs.make('Stack-v0', n_parallel=6, seed=2, pool=ref_pool, episode_length=5, block=True)
  obs, _, _ = env.reset()
  for _ in range(3):
    obs, _, _ = env.step(env.sample())
  for method in ('height', 'difference', 'corrcoef', 'correlate'):
    pol = Bd.Baseline(method=method, goal=True, minorder=1)
    acts = pol(obs).cpu().numpy()
    om, oo = obs[0].cpu().numpy(), obs[1].cpu().numpy()
    for i in range(6):
      inp = (om[i], oo[i])
      vals = B.METHODS[method](inp)
      a, _ = B.select(vals, B.goal_overlap(inp), True, 1)
      if a != acts[i]:     # float64 sums differ in the last bits between numpy and the kernel: accept exact ties only
        assert abs(vals.flat[a] - vals.flat[acts[i]]) <= 1e-12 * max(1.0, abs(vals.flat[a])), (method, i)
  with pytest.raises(ValueError):
    Bd.Baseline(method='nope')                       # baselines.py:184-187
  env.close()


# ---- the kernels beyond the one golden shape (csrc/heuristics.hip)

def _cuda(torch, maps, objs):
  return (torch.from_numpy(np.ascontiguousarray(maps)).cuda(), torch.from_numpy(np.ascontiguousarray(objs)).cuda())


@pytest.mark.gpu
def test_hip_edges_values_and_masks(edges):
  """Every row of the edge fixture, one observation per launch and stacked per shape (a different goal maximum in every
  env): the two are bit-identical (a workgroup sees nothing of its neighbours) and both match the reference."""
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  pow_dev = []
  for (H, h), names in sorted(_groups(edges).items()):
    inp = _cuda(torch, np.stack([edges[n + '/map'] for n in names]), np.stack([edges[n + '/obj'] for n in names]))
    for name, fn, kw in CASES + POW_CASES:
      vals, mask = Bd.heuristic_values(fn, inp, **kw)
      vals, mask = vals.cpu().numpy(), mask.cpu().numpy()
      for i, n in enumerate(names):
        v1, m1 = Bd.heuristic_values(fn, (inp[0][i:i + 1], inp[1][i:i + 1]), **kw)
        assert np.array_equal(v1.cpu().numpy()[0], vals[i]) and np.array_equal(m1.cpu().numpy()[0], mask[i]), (n, name)
        _check_values(fn, kw, vals[i], edges[n + '/' + name], (n, name), pow_dev)
        assert np.array_equal(mask[i], edges[n + '/goal_overlap_t075']), (n, name)
    for t in THRESHOLDS:
      mask = Bd.heuristic_values('height', inp, threshold=t)[1].cpu().numpy()
      for i, n in enumerate(names):
        m1 = Bd.heuristic_values('height', (inp[0][i:i + 1], inp[1][i:i + 1]), threshold=t)[1].cpu().numpy()
        assert np.array_equal(m1[0], mask[i]), (n, t)
        assert np.array_equal(mask[i], edges['{}/goal_overlap_t{:03d}'.format(n, int(100 * t))]), (n, t)
  print('largest relative deviation of a pow row from the edge golden: {:.3e}'.format(max(pow_dev)))


RANDOM_ROWS = ([('height', {}), ('correlate', {}), ('corrcoef', dict(localized=False)), ('corrcoef', dict(localized=True))]
               + [('difference', dict(difference_exponent=e, weights_exponent=w)) for e in (1, 2, 3) for w in (0, 1, 2, 3)])


@pytest.mark.gpu
@pytest.mark.parametrize('H,h,batch', [(64, 16, 7), (32, 8, 300), (128, 32, 3)])
def test_hip_random_shapes_match_oracle(H, h, batch):
  """Seeded observations with a goal value of their own each, against the oracle: every method, `difference` at every
  exponent pair of {1,2,3} x {0,1,2,3}, both `localized`, four thresholds.  300 envs are more workgroups than CUs."""
  torch = pytest.importorskip('torch')
  from oracle import baselines_oracle as B
  from stackrl_amd import baselines as Bd
  make_obs = _make_obs()
  rng = np.random.RandomState(1000 * H + h)
  obs = [make_obs(rng, H, h, goal=int(rng.randint(1, 256))) for _ in range(batch)]
  inp = _cuda(torch, np.stack([m for m, _ in obs]), np.stack([o for _, o in obs]))
  got = {}
  for r, (fn, kw) in enumerate(RANDOM_ROWS):
    got[r] = Bd.heuristic_values(fn, inp, mask=False, **kw)
  masks = {t: Bd.heuristic_values('height', inp, threshold=t)[1] for t in THRESHOLDS}
  got = {r: v.cpu().numpy() for r, v in got.items()}
  masks = {t: v.cpu().numpy() for t, v in masks.items()}
  with ThreadPoolExecutor(8 if H > 32 else 4) as pool:   # numpy releases the GIL on large maps: the oracle's rows side by side
    ref = list(pool.map(lambda ri: B.METHODS[RANDOM_ROWS[ri[0]][0]](obs[ri[1]], **RANDOM_ROWS[ri[0]][1]),
                        [(r, i) for r in range(len(RANDOM_ROWS)) for i in range(batch)]))
  pow_dev = []
  for r, (fn, kw) in enumerate(RANDOM_ROWS):
    for i in range(batch):
      _check_values(fn, kw, got[r][i], ref[r * batch + i], (fn, kw, i), pow_dev)
  for t in THRESHOLDS:
    for i in range(batch):
      assert np.array_equal(masks[t][i], B.goal_overlap(obs[i], threshold=t)), (t, i)
  print('largest relative deviation of a pow row from the oracle at {}/{}: {:.3e}'.format(H, h, max(pow_dev)))


def _select_maps(OH):
  """Hand-built (values, mask, what) for one map size."""
  rng = np.random.RandomState(OH)
  A = OH * OH
  out = []
  for sign, what in ((1.0, 'positive'), (-1.0, 'negative')):     # the zero border: no border cell is a minimum / every one may be
    v = sign * rng.uniform(0.5, 1.5, (OH, OH))
    m = rng.rand(OH, OH) < 0.5
    m.flat[rng.randint(A)] = True
    out.append((v, m, what))
  v = rng.standard_normal((OH, OH))
  m = rng.rand(OH, OH) < 0.3
  m.flat[rng.randint(A)] = True
  v.flat[np.flatnonzero(~m)[:1]] = 50.0                           # the largest value is not a masked one: masked_max + 0.001
  out.append((v, m, 'mixed'))
  v = 1.0 + np.arange(A, dtype=np.float64).reshape(OH, OH)        # a ramp: no local minimum anywhere -> the fallback
  m = np.zeros((OH, OH), bool)
  m.flat[[A // 2, A - 1]] = True
  out.append((v, m, 'fallback'))
  if A > 256 * 5 + 133:
    for lo, hi, what in ((3, 3 + 256 * 5 + 130, 'tie, lower index in the lower thread'),
                         (200, 256 * 5 + 5, 'tie, lower index in the higher thread')):   # threads 3 | 133 and 200 | 5
      v = rng.uniform(0.5, 1.5, (OH, OH))
      v.flat[[lo, hi]] = -1.0
      assert lo % 256 != hi % 256 and (lo % 256 < 128) != (hi % 256 < 128)
      out.append((v, np.ones((OH, OH), bool), what))
  return out


@pytest.mark.gpu
@pytest.mark.parametrize('OH', [1, 2, 17, 97])
def test_hip_select_on_hand_built_maps(OH):
  """`select` alone on float64 maps uploaded as they are: actions and returned maps bit-exact against the oracle's
  `Baseline.call` at minorder 0-3, with and without the goal mask."""
  torch = pytest.importorskip('torch')
  from oracle import baselines_oracle as B
  from stackrl_amd import baselines as Bd
  maps = _select_maps(OH)
  vals = torch.from_numpy(np.stack([v for v, _, _ in maps])).cuda()
  mask = torch.from_numpy(np.stack([m for _, m, _ in maps])).cuda()
  for mo in (0, 1, 2, 3):
    a, neg = Bd.select(vals, mask, goal=True, minorder=mo, value=True)
    a2 = Bd.select(vals, mask, goal=True, minorder=mo)
    assert torch.equal(a, a2)
    a, neg = a.cpu().numpy(), neg.cpu().numpy()
    for i, (v, m, what) in enumerate(maps):
      ra, rneg = B.select(v, m, True, mo)
      assert a[i] == ra, (what, mo, a[i], ra)
      assert np.array_equal(neg[i], rneg), (what, mo)
      if what == 'fallback' and mo:
        assert ra == OH * OH // 2 and not np.any(B._minimum_filter_const0(v, 1 + 2 * mo)[m] == v[m])
      if what.startswith('tie'):
        assert ra == min(np.flatnonzero(v == -1.0))
  for mo in (0, 2):
    a, neg = Bd.select(vals, None, goal=False, minorder=mo, value=True)
    a, neg = a.cpu().numpy(), neg.cpu().numpy()
    for i, (v, m, what) in enumerate(maps):
      ra, rneg = B.select(v, None, False, mo)
      assert a[i] == ra and np.array_equal(neg[i], rneg), (what, mo)
  with pytest.raises(ValueError):
    Bd.select(vals, None, goal=True)


@pytest.mark.gpu
def test_baseline_policy_chained_without_tie_exemption(gold, edges):
  """The policy's action is the oracle's selection on the kernel's own value map and mask: the same doubles on both
  sides, so no case is left out.  The product's start policy is ('height', minorder 0, threshold 1.0)."""
  torch = pytest.importorskip('torch')
  from oracle import baselines_oracle as B
  from stackrl_amd import baselines as Bd
  batches = [_cuda(torch, gold['obs_map'], gold['obs_obj'])]
  for (H, h), names in sorted(_groups(edges).items()):
    batches.append(_cuda(torch, np.stack([edges[n + '/map'] for n in names]), np.stack([edges[n + '/obj'] for n in names])))
  for inp in batches:
    for method, mo, t in [('height', 0, 1.0)] + [(m, mo, t) for m in SELECT_METHODS for mo, t in ((1, 0.75), (2, 1.0), (3, 0.5))]:
      acts = Bd.Baseline(method, goal=True, minorder=mo, threshold=t)(inp).cpu().numpy()
      vals, mask = Bd.heuristic_values(method, inp, threshold=t)
      vals, mask = vals.cpu().numpy(), mask.cpu().numpy()
      for i in range(len(acts)):
        assert acts[i] == B.select(vals[i], mask[i], True, mo)[0], (tuple(inp[0].shape), method, mo, t, i)
      if mo == 1:
        acts = Bd.Baseline(method, goal=False, minorder=mo)(inp).cpu().numpy()
        assert np.array_equal(acts, vals.reshape(len(acts), -1).argmin(axis=1)), (method, 'goal=False')


def _rows_apart_from(torch, Bd, inp, k):
  """Values, masks and actions of every method, of all envs but env k."""
  keep = [i for i in range(inp[0].shape[0]) if i != k]
  out = []
  for name, fn, kw in CASES + POW_CASES[:1]:
    vals, mask = Bd.heuristic_values(fn, inp, threshold=1.0, **kw)
    acts = Bd.Baseline(fn, goal=True, minorder=1, threshold=1.0, **kw)(inp)
    out.append((name, vals[keep].cpu().numpy(), mask[keep].cpu().numpy(), acts[keep].cpu().numpy(), vals[k].cpu().numpy(), mask[k].cpu().numpy()))
  return out


@pytest.mark.gpu
@pytest.mark.parametrize('what', ['empty object map', 'no goal'])
def test_degenerate_env_leaves_its_batch_untouched(gold, edges, what):
  """One env of a batch with an all-zero object map (Stack-v2 with ordering freedom feeds such rows and discards them),
  or without a goal (gmax = 0: the reference divides by zero, the device returns NaN / inf for that env): the other
  envs' values, masks and actions are bit-identical to the same batch without it."""
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  names = _groups(edges)[(32, 8)]
  for maps, objs, k in ((gold['obs_map'], gold['obs_obj'], 2),
                        (np.stack([edges[n + '/map'] for n in names]), np.stack([edges[n + '/obj'] for n in names]), 0)):
    base = _rows_apart_from(torch, Bd, _cuda(torch, maps, objs), k)
    maps, objs = maps.copy(), objs.copy()
    if what == 'empty object map':
      objs[k] = 0
    else:
      maps[k, :, :, 1] = 0
    for (name, v0, m0, a0, _, _), (_, v1, m1, a1, vk, mk) in zip(base, _rows_apart_from(torch, Bd, _cuda(torch, maps, objs), k)):
      assert np.array_equal(v0, v1) and np.array_equal(m0, m1) and np.array_equal(a0, a1), (what, name)
      if what == 'empty object map':
        assert mk.all(), name                                      # goal_overlap is 0 >= 0 everywhere
        if name == 'height':
          assert np.array_equal(vk, np.zeros_like(vk))


@pytest.mark.gpu
def test_map_larger_than_lds_is_refused_before_launch():
  """H = 256, h = 64 (resolution_factor 6) needs 173,056 bytes of LDS per workgroup, more than a CU has: the host
  refuses the call, says why, launches nothing and leaves the device usable."""
  import ctypes
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  xm = torch.zeros((2, 256, 256, 2), dtype=torch.uint8, device='cuda')
  xo = torch.zeros((2, 64, 64, 1), dtype=torch.uint8, device='cuda')
  with pytest.raises(RuntimeError, match=r'H = 256, h = 64 needs 173056 bytes of LDS'):
    Bd.heuristic_values('height', (xm, xo))
  vals = torch.full((2, 193, 193), -7.0, dtype=torch.float64, device='cuda')
  mask = torch.full((2, 193, 193), 9, dtype=torch.uint8, device='cuda')
  L = Bd.qops.load()
  rc = L.srl_heuristic(2, xm.data_ptr(), xo.data_ptr(), vals.data_ptr(), mask.data_ptr(), 2, 256, 64, 2, 2, 0, 0.75,
                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  torch.cuda.synchronize()
  assert rc == 1 and b'173056' in L.srl_qnet_last_error()
  assert bool((vals == -7.0).all()) and bool((mask == 9).all())    # nothing ran
  v, m = Bd.heuristic_values('height', (xm[:, :64, :64].contiguous(), xo[:, :16, :16].contiguous()))
  assert bool((v == 0).all()) and bool(m.all())
  with pytest.raises(RuntimeError, match='srl_heuristic: bad arguments'):    # the host's message reaches the caller
    Bd.heuristic_values(9, (xm[:, :64, :64].contiguous(), xo[:, :16, :16].contiguous()))
