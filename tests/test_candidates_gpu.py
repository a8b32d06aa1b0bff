"""GPU tests of libstackrl_candidates.so: `cand` and `count` equal tests/candidates_cases.py's restatement of
include/stackrl_candidates.h bit for bit over the list of cases, at radius 0 the kernel gives `lookahead.candidates`, the
refusals leave the outputs alone, and `LookaheadPolicy(radius=...)` evaluates the restatement's candidates on real envs."""
import numpy as np
import pytest
import torch

import candidates_cases as cases

pytestmark = pytest.mark.gpu

CASES = cases.cases()
SENTINEL = -77


def _device(case, v, a, stream=None):
  from stackrl_amd import candidates
  dev = torch.device('cuda', 0)
  values = torch.as_tensor(v).to(dev)
  action = None if a is None else torch.as_tensor(a).to(dev)
  if stream is None:
    cand, count = candidates.select(values, action, k=case.k, radius=case.radius, n_valid=case.n_valid, OH=case.OH)
  else:
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
      cand, count = candidates.select(values, action, k=case.k, radius=case.radius, n_valid=case.n_valid, OH=case.OH)
    stream.synchronize()
  assert cand.dtype == torch.int64 and count.dtype == torch.int32 and tuple(cand.shape) == (case.B, case.k) and tuple(count.shape) == (case.B,)
  return cand.cpu().numpy(), count.cpu().numpy()


def test_the_cases_cover_what_the_kernel_turns_on():
  """One kernel, one path; what it branches on is the number of entries against the workgroup (a thread with no entry, one
  entry, several, and the four-fold unrolled pass beyond three passes), the element type, the action and exhaustion."""
  T = cases.THREADS
  n = {c.n_valid * c.OH * c.OH for c in CASES}
  assert min(n) < 64 and any(64 < x < T and x % 64 for x in n) and any(T < x <= 3 * T for x in n)
  assert any(x > 3 * T and (x - 3 * T) % (4 * T) for x in n) and any(x > 7 * T for x in n)
  assert {c.OH for c in CASES} >= {1, 5, 11, 33, 97}
  assert {(c.G, c.n_valid) for c in CASES} >= {(1, 1), (4, 1), (4, 3), (4, 4)} and {c.B for c in CASES} >= {1, 3, 130}
  for OH in (5, 11, 33, 97):
    assert {(c.radius, c.k) for c in CASES if c.OH == OH} >= {(r, k) for r in (0, 1, 4, OH + 1) for k in (1, 2, 8, 32)}
  assert {(c.radius, c.k) for c in CASES if c.OH == 1 and c.G == 3} >= {(0, 1), (0, 2), (0, 3), (1, 3)}
  assert {c.dtype for c in CASES} == {'float32', 'float64'}
  assert {c.values for c in CASES} >= {'constant', 'quantised', 'edge', 'neginf', 'nan', 'close', 'smooth', 'random'}
  assert {c.action for c in CASES} == {'none', 'random', 'corners', 'beyond', 'outside'}
  c = next(c for c in CASES if c.action == 'corners' and c.B >= 4)
  assert set(cases.inputs(c)[1] % (c.OH * c.OH)) == {0, c.OH - 1, c.OH * c.OH - c.OH, c.OH * c.OH - 1}
  c = next(c for c in CASES if c.action == 'outside')
  a = cases.inputs(c)[1]
  assert a.min() < 0 and a.max() >= c.G * c.OH * c.OH
  # exhaustion is reached (count < k), and so is a full list at a radius > 0
  counts = [cases.reference(*cases.inputs(c), c.k, c.radius, c.n_valid, c.OH)[1] for c in CASES if c.OH <= 11]
  ks = [c.k for c in CASES if c.OH <= 11]
  assert any((n < k).any() for n, k in zip(counts, ks)) and any((n == k).all() and k == 32 for n, k in zip(counts, ks))


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_candidates_equal_the_restatement(case):
  v, a = cases.inputs(case)
  want = cases.reference(v, a, case.k, case.radius, case.n_valid, case.OH)
  got = _device(case, v, a)
  assert np.array_equal(got[1], want[1]), 'count'
  assert np.array_equal(got[0], want[0]), 'cand'


def test_on_a_stream_of_its_own_and_twice_the_same():
  case = next(c for c in CASES if c.OH == 97 and c.radius == 4 and c.k == 8 and c.dtype == 'float32')
  v, a = cases.inputs(case)
  want = cases.reference(v, a, case.k, case.radius, case.n_valid, case.OH)
  first = _device(case, v, a, stream=torch.cuda.Stream())
  again = _device(case, v, a, stream=torch.cuda.Stream())
  for got in (first, again):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
def test_radius_0_is_lookahead_candidates_on_device_tensors(dtype):
  from stackrl_amd import candidates
  from stackrl_amd import lookahead as la
  dev = torch.device('cuda', 0)
  for kind, (G, n_valid, OH), k, where in (('smooth', (1, 1, 97), 8, 'random'), ('quantised', (4, 3, 11), 32, 'random'),
                                           ('nan', (4, 3, 11), 8, 'beyond'), ('neginf', (2, 2, 33), 2, 'corners'),
                                           ('close', (1, 1, 11), 8, 'random'), ('constant', (1, 1, 5), 1, 'random')):
    B = 5
    raw = cases.make_values(kind, B, G, OH, dtype, 3)
    action = torch.as_tensor(cases.make_action(where, B, G, OH, n_valid, 3)).to(dev)
    # every NaN, whatever its sign bit: the function on CPU copies (point 5 of the header: `torch.sort` on the device ranks a
    # NaN with the sign bit set last, on the CPU first, as the definition does)
    cand, count = candidates.select(torch.as_tensor(raw).to(dev), action, k=k, radius=0, n_valid=n_valid, OH=OH)
    assert torch.equal(cand.cpu(), la.candidates(action.cpu(), torch.as_tensor(raw), k, n_valid, OH * OH)), (kind, G, n_valid, OH, k)
    # the same tensors on the device, the NaNs with the sign bit clear
    values = torch.as_tensor(np.where(np.isnan(raw), np.asarray(np.nan, raw.dtype), raw)).to(dev)
    assert not bool((torch.isnan(values) & (values.view(torch.int32 if dtype == 'float32' else torch.int64) < 0)).any())
    want = la.candidates(action, values, k, n_valid, OH * OH)
    cand, count = candidates.select(values, action, k=k, radius=0, n_valid=n_valid, OH=OH)
    assert torch.equal(cand, want), (kind, G, n_valid, OH, k)
    assert count.tolist() == [k] * B
    ref = candidates.select_reference(values, action, k=k, radius=0, n_valid=n_valid, OH=OH)
    assert torch.equal(ref[0], want) and torch.equal(ref[1], count)


def test_other_dtypes_and_strides_go_as_contiguous_float32():
  from stackrl_amd import candidates
  dev = torch.device('cuda', 0)
  half = torch.as_tensor(cases.make_values('smooth', 3, 2, 11, 'float32', 9)).to(dev).to(torch.bfloat16)
  strided = half.reshape(3, 2, 11, 11).permute(0, 1, 3, 2)                        # transposed maps: not contiguous
  for t in (half, strided):
    want = cases.reference(t.float().reshape(3, -1).cpu().numpy(), None, 8, 2, 2, 11)
    got = candidates.select(t, k=8, radius=2, n_valid=2, OH=11)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


def test_refusals_return_their_codes_and_leave_the_outputs_unwritten():
  from stackrl_amd import candidates
  dev = torch.device('cuda', 0)
  lib = candidates.load()
  values = torch.rand(2, 50, device=dev)
  cand = torch.full((2, 32), SENTINEL, dtype=torch.int64, device=dev)
  count = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)
  good = dict(B=2, G=2, OH=5, n_valid=2, k=4, radius=1)
  for bad, word in ((dict(B=0), 'B must'), (dict(G=0), 'G must'), (dict(OH=0), 'OH must'), (dict(n_valid=3), 'n_valid must'),
                    (dict(k=0), 'k must'), (dict(k=33), 'k must'), (dict(radius=-1), 'radius must')):
    p = dict(good, **bad)
    rc = lib.srl_candidates_select(values.data_ptr(), 0, None, p['B'], p['G'], p['OH'], p['n_valid'], p['k'], p['radius'],
                                   cand.data_ptr(), count.data_ptr(), None)
    assert rc == 1 and word in lib.srl_candidates_last_error().decode()
    with pytest.raises(RuntimeError, match=word):
      candidates.call('srl_candidates_select', values, values, 0, None, p['B'], p['G'], p['OH'], p['n_valid'], p['k'], p['radius'], cand, count)
  assert lib.srl_candidates_select(values.data_ptr(), 0, None, 2, 2, 5, 2, 4, 1, None, count.data_ptr(), None) == 1
  torch.cuda.synchronize()
  assert bool((cand == SENTINEL).all()) and bool((count == SENTINEL).all())
  # and a good call after them writes exactly [B][k] and [B]
  candidates.call('srl_candidates_select', values, values, 0, None, 2, 2, 5, 2, 4, 1, cand, count)
  want = cases.reference(values.cpu().numpy(), None, 4, 1, 2, 5)
  assert np.array_equal(cand.reshape(-1)[:8].reshape(2, 4).cpu().numpy(), want[0]) and bool((cand.reshape(-1)[8:] == SENTINEL).all())
  assert np.array_equal(count.cpu().numpy(), want[1])


def test_the_policy_on_real_envs(ref_pool):
  from stackrl_amd import env as envs
  from stackrl_amd import lookahead as la
  from stackrl_amd.baselines import Baseline
  n, L, k = 4, 8, 4
  g = envs.VecStackEnv(n_parallel=n, seed=2, pool=ref_pool, block=True, episode_length=L)
  look = la.Lookahead(g, k)
  base = Baseline('height', value=True)
  plain, zero, spread = la.LookaheadPolicy(base, look), la.LookaheadPolicy(base, look, radius=0), la.LookaheadPolicy(base, look, radius=3)
  obs = g.reset()[0]
  OH = obs[0].shape[1] - obs[1].shape[-3] + 1
  for t in range(3):
    a_plain, _ = plain(obs)
    a_zero, v_zero = zero(obs)
    assert torch.equal(a_plain, a_zero) and torch.equal(plain.last[0], zero.last[0]) and zero.last_count.tolist() == [k] * n
    a0, v0 = base(obs)
    a, v = spread(obs)
    assert torch.equal(v, v0) and torch.equal(v_zero, v0)
    cand, reward = spread.last
    want = cases.reference(v0.reshape(n, -1).cpu().numpy(), a0.cpu().numpy(), k, 3, 1, OH)
    assert np.array_equal(cand.cpu().numpy(), want[0]) and np.array_equal(spread.last_count.cpu().numpy(), want[1])
    assert torch.equal(a, la.choose(cand, reward.to(cand.device)))
    assert torch.equal(reward, look.evaluate(cand)[0])                  # the lookahead leaves the env where it was
    obs = g.step(a)[0]
  look.close()
  g.close()
