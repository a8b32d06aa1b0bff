"""GPU tests of the heuristic baselines on the grouped observation of Stack-v2 (include/stackrl_baseline_rows.h;
csrc/heuristics.hip `k_heuristic_rows`, `k_baseline_rows_select`): the rows bit for bit against `srl_heuristic` on the
expanded observation, the choice exactly against `baselines.baseline_rows_reference` fed with the kernel's own maps, the
reference's own results on the fixture, the composition the parent commit offered, ties, independence of the batch, and the
policy end to end on a Stack-v2 env.  Every output buffer is filled with a sentinel before the call under test."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'baselines_v2_golden.npz')
SENT = -7.0            # values / chosen / neg sentinel
MSENT = 9              # mask sentinel
# (H, h, B, G): one window at (16, 16), four at (33, 32), more windows than threads at (32, 8) on; the product's map once
SHAPES = [(32, 8, 3, 8), (16, 16, 1, 3), (33, 32, 3, 2), (48, 16, 1, 1), (128, 32, 2, 2)]


def _n_valids(G):
  return sorted({1, max(1, G - 1), G})


def _obs(H, h, B, G, seed=0, goal=True):
  """Seeded observations: a rough pile, a goal rectangle with an env's own goal value, G different object maps."""
  rng = np.random.RandomState(1000 * H + 10 * G + B + seed)
  m = np.zeros((B, H, H, 2), np.uint8)
  m[..., 0] = rng.randint(0, 90, (B, H, H)) * (rng.rand(B, H, H) < 0.6)
  for b in range(B):
    u, v = rng.randint(0, max(1, H // 4), 2)
    m[b, u:u + max(h, H // 2), v:v + max(h, H // 2), 1] = rng.randint(100, 256)
  o = (rng.randint(1, 120, (B, G, h, h, 1)) * (rng.rand(B, G, h, h, 1) < 0.7)).astype(np.uint8)
  o[:, :, h // 2, h // 2] = 50                                    # never an empty object map
  return m, o


def _dev(torch, *arrays):
  return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _stream(torch):
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows_call(torch, Bd, method, xm, xo, n_valid, dexp=2, wexp=2, localized=0, threshold=0.75):
  """srl_heuristic_rows into sentinel-filled buffers -> (rc, values, mask)."""
  B, G, h, H = xo.shape[0], xo.shape[1], xo.shape[2], xm.shape[1]
  OH = H - h + 1
  vals = torch.full((B, G, OH, OH), SENT, dtype=torch.float64, device='cuda')
  mask = torch.full((B, G, OH, OH), MSENT, dtype=torch.uint8, device='cuda')
  rc = Bd.qops.load().srl_heuristic_rows(Bd.METHODS[method], xm.data_ptr(), xo.data_ptr(), vals.data_ptr(), mask.data_ptr(), B, G, n_valid,
                                    H, h, dexp, wexp, localized, threshold, _stream(torch))
  torch.cuda.synchronize()
  return rc, vals, mask


def _select_call(torch, Bd, vals, mask, goal, minorder, n_valid):
  """srl_baseline_rows_select into sentinel-filled buffers -> (rc, actions, chosen, neg)."""
  B, G, OH = vals.shape[0], vals.shape[1], vals.shape[-1]
  actions = torch.full((B,), -5, dtype=torch.int64, device='cuda')
  chosen = torch.full((B, G), SENT, dtype=torch.float64, device='cuda')
  neg = torch.full(tuple(vals.shape), SENT, dtype=torch.float64, device='cuda')
  rc = Bd.qops.load().srl_baseline_rows_select(vals.data_ptr(), mask.data_ptr() if mask is not None else None, int(goal), minorder, B, G,
                                          n_valid, OH, actions.data_ptr(), chosen.data_ptr(), neg.data_ptr(), _stream(torch))
  torch.cuda.synchronize()
  return rc, actions, chosen, neg


ROW_CONFIGS = [('height', {}), ('correlate', {}), ('corrcoef', dict(localized=0)), ('corrcoef', dict(localized=1)),
               ('difference', dict(dexp=2, wexp=2)), ('difference', dict(dexp=1, wexp=0)), ('difference', dict(dexp=3, wexp=1)),
               ('height', dict(threshold=1.0)), ('height', dict(threshold=0.0))]


@pytest.mark.parametrize('H,h,B,G', SHAPES)
def test_rows_are_srl_heuristic_on_the_expanded_observation(H, h, B, G):
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd, policies
  xm, xo = _dev(torch, *_obs(H, h, B, G))
  em, eo = policies.expand_orientations((xm, xo))
  for method, kw in (ROW_CONFIGS if H < 128 else ROW_CONFIGS[:1] + ROW_CONFIGS[4:5]):
    ref_v, ref_m = Bd.heuristic_values(method, (em.contiguous(), eo.contiguous()), difference_exponent=kw.get('dexp', 2),
                                       weights_exponent=kw.get('wexp', 2), localized=kw.get('localized', 0),
                                       threshold=kw.get('threshold', 0.75))
    ref_v = ref_v.reshape(B, G, *ref_v.shape[1:]); ref_m = ref_m.reshape(B, G, *ref_m.shape[1:]).to(torch.uint8)
    for n_valid in (_n_valids(G) if method in ('height', 'difference') and not kw.get('threshold') else [G]):
      rc, vals, mask = _rows_call(torch, Bd, method, xm, xo, n_valid, **kw)
      assert rc == 0
      assert vals[:, :n_valid].view(torch.int64).equal(ref_v[:, :n_valid].view(torch.int64)), (method, kw, n_valid)   # bit for bit
      assert mask[:, :n_valid].equal(ref_m[:, :n_valid]), (method, kw, n_valid)
      assert bool((vals[:, n_valid:] == SENT).all()) and bool((mask[:, n_valid:] == MSENT).all()), (method, kw, n_valid)


@pytest.mark.parametrize('H,h,B,G', SHAPES)
def test_selection_is_the_restatement_on_the_kernels_own_maps(H, h, B, G):
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  xm, xo = _dev(torch, *_obs(H, h, B, G, seed=1))
  for method in ('height', 'difference') if H < 128 else ('height',):
    vals, mask = Bd.heuristic_values(method, (xm, xo))
    mk8 = mask.to(torch.uint8)
    for n_valid in _n_valids(G):
      for goal in (True, False):
        for mo in (0, 1, 2):
          rc, actions, chosen, neg = _select_call(torch, Bd, vals, mk8 if goal else None, goal, mo, n_valid)
          assert rc == 0
          ra, rc_, rneg = Bd.baseline_rows_reference(vals, mask, goal=goal, minorder=mo, n_valid=n_valid)
          what = (method, n_valid, goal, mo)
          assert np.array_equal(actions.cpu().numpy(), ra), what
          assert np.array_equal(chosen.cpu().numpy(), rc_), what
          assert np.array_equal(neg.cpu().numpy(), rneg), what
          assert np.isneginf(chosen.cpu().numpy()[:, n_valid:]).all() and np.isneginf(neg.cpu().numpy()[:, n_valid:]).all(), what
          # the Python surface: the same results through `select`
          a2, c2, n2 = Bd.select(vals, mask if goal else None, goal=goal, minorder=mo, value=True, n_valid=n_valid, chosen=True)
          assert a2.equal(actions) and c2.equal(chosen) and n2.equal(neg), what


def _composition(torch, Bd, policies, method, inputs, goal, minorder, n_valid=None, **kw):
  """What the parent commit could do: expand, the per-sample kernels, then the row choice in torch."""
  xm, xo = inputs
  B, G = xo.shape[0], xo.shape[1]
  em, eo = policies.expand_orientations((xm, xo))
  out = Bd.heuristic_values(method, (em.contiguous(), eo.contiguous()), mask=goal, **kw)
  vals, mask = out if goal else (out, None)
  a, neg = Bd.select(vals, mask, goal=goal, minorder=minorder, value=True)
  A = vals.shape[1] * vals.shape[2]
  c = neg.reshape(B * G, A).gather(1, a[:, None]).reshape(B, G)
  if n_valid is not None:
    c[:, n_valid:] = -float('inf')
  row = torch.argmax(c, dim=1)                                    # ties to the first row
  return row * A + a.reshape(B, G).gather(1, row[:, None])[:, 0]


def test_fixture_actions_and_the_parent_style_composition():
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd, policies
  fix = np.load(FIX)
  for tag in fix['shapes']:
    inp = _dev(torch, fix[tag + '/obs_map'], fix[tag + '/obs_obj'])
    G = inp[1].shape[1]
    A = (inp[0].shape[1] - inp[1].shape[2] + 1) ** 2
    for method in (str(x) for x in fix['methods']):
      for goal in (True, False):
        for mo in (int(x) for x in fix['minorders']):
          key = '{}/{}/g{}_m{}'.format(tag, method, int(goal), mo)
          actions, neg = Bd.Baseline(method, goal=goal, minorder=mo, value=True)(inp)
          assert neg.shape == (inp[0].shape[0], G * A)
          assert np.array_equal(actions.cpu().numpy(), fix[key + '/row'] * A + fix[key + '/action']), key
          assert actions.equal(Bd.Baseline(method, goal=goal, minorder=mo)(inp)), key
          assert actions.equal(_composition(torch, Bd, policies, method, inp, goal, mo)), key
      k = G - 1
      assert Bd.Baseline(method)(inp, n_valid=k).equal(_composition(torch, Bd, policies, method, inp, True, 1, n_valid=k)), (tag, method)


def test_ties_between_rows_on_the_device():
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  from test_baseline_rows import tie_cases
  for what, v, row in tie_cases():
    for goal, mo in ((True, 1), (True, 0), (False, 1)):
      vals = torch.from_numpy(v).cuda()
      mask = torch.ones(v.shape, dtype=torch.uint8, device='cuda')
      rc, actions, chosen, neg = _select_call(torch, Bd, vals, mask, goal, mo, v.shape[1])
      assert rc == 0 and int(actions[0]) == row * 9 + 4, (what, goal, mo)
  # a tie between rows 1 and 2 in the last env of a batch of 3: the earlier envs have a best row of their own
  rng = np.random.RandomState(5)
  v = 1.0 + rng.rand(3, 4, 5, 5)
  v[0, 3, 2, 2] = 0.5; v[1, 0, 1, 3] = 0.5
  v[2, 1, 3, 1] = 0.25; v[2, 2, 2, 2] = 0.25
  vals = torch.from_numpy(v).cuda()
  mask = torch.ones(v.shape, dtype=torch.uint8, device='cuda')
  for goal, mo in ((True, 1), (True, 0), (False, 0)):
    rc, actions, chosen, neg = _select_call(torch, Bd, vals, mask, goal, mo, 4)
    assert rc == 0 and actions.tolist() == [3 * 25 + 12, 0 * 25 + 8, 1 * 25 + 16], (goal, mo, actions.tolist())
    assert np.array_equal(actions.cpu().numpy(), Bd.baseline_rows_reference(v, np.ones(v.shape, bool), goal, mo)[0])


def test_batch_and_row_independence():
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  H, h, B, G = 32, 8, 3, 8
  m, o = _obs(H, h, B, G, seed=2)
  xm, xo = _dev(torch, m, o)
  for method in ('height', 'difference', 'corrcoef'):
    pol = Bd.Baseline(method, value=True)
    a, neg = pol((xm, xo))
    for b in range(B):                                             # a batch of 3 = three single calls
      a1, neg1 = pol((xm[b:b + 1], xo[b:b + 1]))
      assert a1.equal(a[b:b + 1]) and neg1.view(torch.int64).equal(neg[b:b + 1].view(torch.int64)), (method, b)
    a3, neg3 = pol((xm, xo), n_valid=3)                            # G = 8 with n_valid = 3 = G = 3
    b3, nb3 = pol((xm, xo[:, :3].contiguous()))
    A = (H - h + 1) ** 2
    assert a3.equal(b3) and neg3[:, :3 * A].view(torch.int64).equal(nb3.view(torch.int64)), method
    assert bool(torch.isneginf(neg3[:, 3 * A:]).all())
  # an env without a goal in the middle of the batch: its neighbours' results do not change
  m2 = m.copy(); m2[1, :, :, 1] = 0
  xm2, = _dev(torch, m2)
  for method in ('height', 'correlate'):
    a, neg = Bd.Baseline(method, value=True)((xm, xo))
    a2, neg2 = Bd.Baseline(method, value=True)((xm2, xo))
    keep = [0, 2]
    assert a2[keep].equal(a[keep]) and neg2[keep].view(torch.int64).equal(neg[keep].view(torch.int64)), method
  # 'random': one draw for all B * G maps from the policy's generator, the kernel's masks
  pol = Bd.Baseline('random', seed=3, value=True)
  a, neg = pol((xm, xo))
  gen = torch.Generator(device='cuda'); gen.manual_seed(3)
  A = (H - h + 1) ** 2
  vals = torch.rand((B, G, H - h + 1, H - h + 1), generator=gen, device='cuda', dtype=torch.float64)
  mask = Bd.heuristic_values('height', (xm, xo))[1]
  ra, _, rneg = Bd.baseline_rows_reference(vals, mask)
  assert np.array_equal(a.cpu().numpy(), ra) and np.array_equal(neg.cpu().numpy(), rneg.reshape(B, G * A))


def test_refusals_launch_nothing():
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd
  xm, xo = _dev(torch, *_obs(32, 8, 2, 3))
  L = Bd.qops.load()
  for bad in (0, 4, -1):
    rc, vals, mask = _rows_call(torch, Bd, 'height', xm, xo, bad)
    assert rc == 1 and b'srl_heuristic_rows: bad arguments' in L.srl_qnet_last_error()
    assert bool((vals == SENT).all()) and bool((mask == MSENT).all())
    v = torch.rand((2, 3, 25, 25), dtype=torch.float64, device='cuda')
    rc, actions, chosen, neg = _select_call(torch, Bd, v, torch.ones_like(v, dtype=torch.uint8), True, 1, bad)
    assert rc == 1 and b'srl_baseline_rows_select: bad arguments' in L.srl_qnet_last_error()
    assert bool((actions == -5).all()) and bool((chosen == SENT).all()) and bool((neg == SENT).all())
    with pytest.raises(ValueError, match='n_valid'):
      Bd.Baseline('height')((xm, xo), n_valid=bad)
  v = torch.rand((2, 3, 25, 25), dtype=torch.float64, device='cuda')
  rc, actions, chosen, neg = _select_call(torch, Bd, v, torch.ones_like(v, dtype=torch.uint8), True, -1, 3)   # minorder < 0
  assert rc == 1 and bool((actions == -5).all()) and bool((neg == SENT).all())
  rc, actions, chosen, neg = _select_call(torch, Bd, v, None, True, 1, 3)                                      # goal without a mask
  assert rc == 1 and bool((actions == -5).all())
  big_m = torch.zeros((1, 256, 256, 2), dtype=torch.uint8, device='cuda')                                     # the LDS refusal
  big_o = torch.zeros((1, 2, 64, 64, 1), dtype=torch.uint8, device='cuda')
  rc, vals, mask = _rows_call(torch, Bd, 'height', big_m, big_o, 2)
  assert rc == 1 and b'H = 256, h = 64 needs 173056 bytes of LDS' in L.srl_qnet_last_error()
  assert bool((vals == SENT).all()) and bool((mask == MSENT).all())
  with pytest.raises(RuntimeError, match='173056 bytes of LDS'):
    Bd.Baseline('height')((big_m, big_o))
  with pytest.raises(ValueError, match='uint8'):
    Bd.Baseline('height')((xm, xo.float()))
  a = Bd.Baseline('height')((xm, xo))                              # the device is as usable as before
  assert a.shape == (2,) and int(a.max()) < 3 * 625


@pytest.mark.parametrize('ordering', [False, True])
def test_baseline_drives_stack_v2_end_to_end(ref_pool, ordering):
  torch = pytest.importorskip('torch')
  from stackrl_amd import baselines as Bd, env as envs
  n, L = 4, 3
  g = envs.make('Stack-v2', n_parallel=n, seed=6, pool=ref_pool, block=True, episode_length=L, orientation_freedom=2,
                ordering_freedom=ordering)
  pol = Bd.Baseline('height', value=True)
  obs, _, _ = g.reset()
  for t in range(3):
    n_valid = g.num_maps_on_show if ordering else None
    a, neg = pol(obs, n_valid=n_valid)
    vals, mask = Bd.heuristic_values('height', obs, n_valid=n_valid)
    ra, _, rneg = Bd.baseline_rows_reference(vals, mask, n_valid=n_valid)
    assert np.array_equal(a.cpu().numpy(), ra) and np.array_equal(neg.cpu().numpy(), rneg.reshape(n, -1)), t
    assert int(a.max()) < g.n_actions
    if ordering:
      assert int((a // 9409).max()) < g.num_maps_on_show
    obs, _, d = g.step(a)                                          # block=True: srl_sync_status raises on a refused action
  assert bool(d.all())
  g.close()
