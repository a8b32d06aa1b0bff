"""GPU tests of the greedy head alone: the kernel `k_greedy_head` (csrc/greedy.hip) against the torch restatement of its
definition (include/stackrl_greedy.h; `stackrl_amd.dqn.greedy_head_reference`).  The shapes are the smallest at which the
kernel can go wrong (one thread's stride is 256 elements, a float4 path for rows of a multiple of four floats), not the
workload's."""
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
NAN, INF = float('nan'), float('inf')


def _case(B, G, A, seed):
  g = torch.Generator(device='cuda').manual_seed(seed)
  return 3 * torch.randn((B, G, A), generator=g, device='cuda'), torch.randn(B, generator=g, device='cuda')


@pytest.mark.parametrize('A', [1, 3, 255, 256, 257, 1025, 9409])
@pytest.mark.parametrize('B,G,n_valid', [(1, 1, 1), (3, 2, 1), (3, 2, 2), (2, 8, 7)])
def test_kernel_against_the_restatement(B, G, n_valid, A):
  from stackrl_amd import qops
  from stackrl_amd.dqn import greedy_head_reference
  adv, v = _case(B, G, A, 100000 * B + 1000 * G + 10 * A + n_valid)
  actions, stats, q = qops.greedy_head(adv, v, n_valid, stats=True, values=True)
  assert actions.shape == (B,) and actions.dtype == torch.int64 and stats.shape == (B, 4) and stats.dtype == torch.float64
  assert q.shape == adv.shape and q.dtype == torch.float32
  assert int(actions.min()) >= 0 and int(actions.max()) < n_valid * A
  a = adv.double()[:, :n_valid]
  m = a.mean(-1)
  q64 = (a - m[..., None] + v.double()[:, None, None]).reshape(B, -1)              # the literal float64 statement
  # one rounding of the mean plus the two float32 operations
  bound = EPS * (m.abs().amax(-1) + a.abs().amax(dim=(1, 2)) + v.double().abs())
  chosen = q64.gather(1, actions[:, None])[:, 0]
  print('shortfall / bound:', ((q64.amax(-1) - chosen) / bound).tolist(), 'same as float64 arg-max:', (actions == q64.argmax(-1)).tolist())
  assert bool((q64.amax(-1) - chosen <= bound).all())
  # q against the restatement on the device: within one float32 unit of |m| + |a| + |v| per element, -inf in the invalid rows
  ra, rs, rq = greedy_head_reference(adv, v, n_valid)
  unit = EPS * (m.abs()[..., None] + a.abs() + v.double().abs()[:, None, None])
  err = (q[:, :n_valid].double() - rq[:, :n_valid].double()).abs()
  print('q: largest error / unit', float((err / unit).max()), 'equal to the restatement bit for bit:', torch.equal(q, rq))
  assert bool((err <= unit).all())
  assert bool(torch.isneginf(q[:, n_valid:]).all()) and q[:, n_valid:].numel() == B * (G - n_valid) * A
  # the statistics are those of the kernel's own q
  flat = q[:, :n_valid].reshape(B, -1)
  assert torch.equal(actions, torch.argmax(flat, dim=-1))
  assert torch.equal(stats[:, 0], flat.amax(-1).double()) and torch.equal(stats[:, 1], flat.amin(-1).double())
  d = flat.double()
  assert bool(((stats[:, 2] - d.sum(-1)).abs() <= 1e-12 * d.abs().sum(-1)).all())
  assert bool(((stats[:, 3] - (d * d).sum(-1)).abs() <= 1e-12 * (d * d).sum(-1)).all())
  # what is not asked for is not returned, and the action does not depend on it
  assert torch.equal(qops.greedy_head(adv, v, n_valid), actions)
  a2, s2 = qops.greedy_head(adv, v, n_valid, stats=True)
  assert torch.equal(a2, actions) and torch.equal(s2, stats)
  if G == 1:
    a3, q3 = qops.greedy_head(adv[:, 0], v, values=True)
    assert torch.equal(a3, actions) and torch.equal(q3, q[:, 0])


@pytest.mark.parametrize('A', [1025, 1028])          # the scalar path and the float4 path
def test_without_a_value_q_is_the_advantage(A):
  from stackrl_amd import qops
  adv, _ = _case(3, 2, A, 7)
  a, st, q = qops.greedy_head(adv, None, stats=True, values=True)
  assert torch.equal(q, adv) and torch.equal(a, torch.argmax(adv.reshape(3, -1), dim=-1))
  assert torch.equal(st[:, 0], adv.amax(dim=(1, 2)).double()) and torch.equal(st[:, 1], adv.amin(dim=(1, 2)).double())


# (G, A, first, second): equal maxima planted at two flat indices; the first must win
TIES = [(1, 1025, 7, 7 + 256),                        # within one thread's stride
        (1, 1025, 9, 300),                            # across threads (and across waves)
        (1, 1028, 5, 6),                              # float4 path: inside one quad
        (1, 2052, 8, 8 + 1024),                       # float4 path: one thread's next quad
        (2, 1025, 0, 1025 + 1024),                    # first element of the first row against the last of the last valid row
        (2, 1028, 0, 1028 + 1027)]


@pytest.mark.parametrize('G,A,i,j', TIES)
def test_ties_go_to_the_lowest_flat_index(G, A, i, j):
  from stackrl_amd import qops
  adv, _ = _case(4, G, A, 5)
  flat = adv.reshape(4, -1)
  flat[:, i] = flat[:, j] = 1e30                      # without a value q = adv: the two are equal
  assert qops.greedy_head(adv, None).tolist() == [i] * 4
  # with the value: the rows' means differ, so the planted pair must sit in one row to stay equal
  if j < A:
    v = torch.randn(4, device='cuda')
    assert qops.greedy_head(adv, v).tolist() == [i] * 4


@pytest.mark.parametrize('A', [257, 1028])
def test_two_identical_rows_tie_into_the_first(A):
  from stackrl_amd import qops
  adv, v = _case(3, 1, A, 6)
  two = adv.expand(3, 2, A).contiguous()              # same mean, same q
  a, q = qops.greedy_head(two, v, values=True)
  assert torch.equal(q[:, 0], q[:, 1])
  assert torch.equal(a, torch.argmax(q[:, 0], dim=-1)) and int(a.max()) < A
  const = torch.full((2, 3, A), 1.25, device='cuda')  # a constant row: every q equals v, the action is 0
  a, q = qops.greedy_head(const, torch.tensor([0.5, -2.0], device='cuda'), values=True)
  assert a.tolist() == [0, 0] and torch.equal(q, torch.tensor([0.5, -2.0], device='cuda')[:, None, None].expand(2, 3, A))


@pytest.mark.parametrize('A', [1, 257, 260])
@pytest.mark.parametrize('fill', [-INF, NAN])
def test_degenerate_rows(A, fill):
  from stackrl_amd import qops
  # as the sole row: nothing wins, the action is 0
  sole = torch.full((2, 1, A), fill, device='cuda')
  for v in (None, torch.zeros(2, device='cuda')):
    a, st = qops.greedy_head(sole, v, stats=True)
    assert a.tolist() == [0, 0]
    assert bool(torch.isneginf(st[:, 0]).all())
  # beside a finite row (either order): the finite row wins
  fin, _ = _case(2, 1, A, 8)
  for order in (0, 1):
    rows = [sole, fin] if order else [fin, sole]
    adv = torch.cat(rows, dim=1).contiguous()
    a, st = qops.greedy_head(adv, None, stats=True)
    assert torch.equal(a, order * A + torch.argmax(fin[:, 0], dim=-1))
    assert torch.equal(st[:, 0], fin[:, 0].amax(-1).double())
    if fill != fill:                                 # NaN is skipped by max and min, not by the sums
      assert torch.equal(st[:, 1], fin[:, 0].amin(-1).double()) and bool(torch.isnan(st[:, 2:]).all())
  # one action
  one, v = _case(5, 1, 1, 9)
  a, q = qops.greedy_head(one, v, values=True)
  assert a.tolist() == [0] * 5 and torch.equal(q[:, 0, 0], (one[:, 0, 0] - one[:, 0, 0]) + v)


@pytest.mark.parametrize('A', [257, 260])
def test_invalid_rows_are_never_read(A):
  from stackrl_amd import qops
  adv, v = _case(3, 4, A, 10)
  ref = qops.greedy_head(adv, v, 2, stats=True, values=True)
  for junk in (NAN, INF):
    dirty = adv.clone()
    dirty[:, 2:] = junk
    got = qops.greedy_head(dirty, v, 2, stats=True, values=True)
    assert all(torch.equal(x, y) for x, y in zip(got, ref))
  assert bool(torch.isneginf(ref[2][:, 2:]).all())


def test_results_belong_to_envs_not_to_the_batch():
  from stackrl_amd import qops
  B, G, A = 64, 2, 2401
  adv, v = _case(B, G, A, 11)
  whole = qops.greedy_head(adv, v, stats=True, values=True)
  s = torch.randperm(B, device='cuda')
  perm = qops.greedy_head(adv[s], v[s], stats=True, values=True)
  assert all(torch.equal(p, w[s]) for p, w in zip(perm, whole))
  halves = [qops.greedy_head(adv[sl], v[sl], stats=True, values=True) for sl in (slice(0, 32), slice(32, B))]
  assert all(torch.equal(torch.cat([halves[0][k], halves[1][k]]), whole[k]) for k in range(3))


def test_bad_arguments_raise_with_the_entry_points_message():
  from stackrl_amd import qops
  adv, v = _case(3, 2, 5, 12)
  for n_valid in (0, 3):
    with pytest.raises(RuntimeError, match='srl_greedy_head: bad arguments'):
      qops.greedy_head(adv, v, n_valid)
  with pytest.raises(RuntimeError, match='srl_greedy_head: bad arguments'):
    qops.greedy_head(torch.empty((3, 2, 0), device='cuda'), v)
  # a value that does not cover the batch never reaches the kernel
  with pytest.raises(ValueError, match='srl_greedy_head'):
    qops.greedy_head(adv, v[:2])
  with pytest.raises(ValueError, match='srl_greedy_head'):
    qops.greedy_head(adv, v.cpu())
  with pytest.raises(ValueError, match=r'\[B, A\] or \[B, G, A\]'):
    qops.greedy_head(adv[0, 0], None)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    qops.greedy_head(adv.cpu(), None)
  assert qops.greedy_head(adv, v).shape == (3,)
