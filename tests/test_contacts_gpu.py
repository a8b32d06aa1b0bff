"""GPU tests of `srl_contact_points` (csrc/contacts.hip; include/stackrl_hip.h "Contact points") through
`VecStackEnv.contact_points`: the kernel against the numpy restatement of tests/contact_cases.py bit for bit on the records
`get_state` returns, capacity and `last`, the states around a reset and the other env classes, that a call changes nothing,
the refusals, and the momentum balance of a sub-step — the check that does not come from the code under test."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import contact_cases as cc

pytestmark = pytest.mark.gpu

N = 4
KW = dict(resolution_factor=4)


def _mk(ref_pool, L, seed=5, cls=None, **kw):
  from stackrl_amd import env as envs
  args = dict(KW, **kw)
  return (cls or envs.VecStackEnv)(n_parallel=N, seed=seed, pool=ref_pool, block=True, episode_length=L, **args)


def _centre(g):
  """The same pixel for every env and every step: rocks land on rocks."""
  aw = g.config.overhead_res - g.config.object_res + 1
  return torch.full((N,), (aw // 2) * aw + aw // 2, dtype=torch.int64, device='cuda')


@pytest.fixture(scope='module')
def verts(ref_pool):
  return cc.com_vertices(ref_pool)


def _bits(a):
  return np.ascontiguousarray(a).view(np.int32)


def _assert_equals_restatement(g, cp, verts, tag, last=False):
  """`cp` (on the host) against the restatement of every env's record; returns the counts."""
  L, dt = g.config.episode_length, np.float32(g.config.sim_time_step)
  rec = g.get_state().records.cpu().numpy()
  C = cp.capacity
  for e in range(N):
    count, b, r, w = cc.decode(rec[e], L, dt, verts, last_only=last, capacity=C, with_wrench=cp.wrench is not None)
    n = min(count, C)
    assert int(cp.count[e]) == count, (tag, e)
    assert np.array_equal(cp.bodies[e, :n].numpy(), b[:n]), (tag, e)
    assert np.array_equal(_bits(cp.rows[e, :n].numpy()), _bits(r[:n])), (tag, e, np.abs(cp.rows[e, :n].numpy() - r[:n]).max())
    if w is not None:
      assert np.array_equal(_bits(cp.wrench[e].numpy()), _bits(w)), (tag, e, np.abs(cp.wrench[e].numpy() - w).max())
  return cp.count.numpy()


# ------------------------------------------------------------------------------------------------ 1. kernel against restatement
@pytest.mark.parametrize('L', [1, 8, 9, 32])
def test_kernel_equals_the_restatement_after_every_step(ref_pool, verts, L):
  """4 NS crosses 64 between the lengths (4, 112, 144, 512 pair candidates), and at 32 the candidates span several chunks.  A
  single rock has neither a pair point nor 64 candidates (8): those two assertions are made where the length admits them."""
  g = _mk(ref_pool, L)
  g.reset()
  a = _centre(g)
  pair_points, most_candidates = 0, 0
  for t in range(L):
    g.step(a)
    cp = g.contact_points(wrench=True).cpu()
    counts = _assert_equals_restatement(g, cp, verts, 'step {}'.format(t))
    pen, npts = g.contacts()
    assert np.array_equal(counts, npts), t
    for e in range(N):
      d = cp.distance[e, :counts[e]].numpy()
      assert np.float32(max([0.0] + list(-d))) == pen[e], (t, e)
      pair_points += int((cp.body_b[e, :counts[e]] >= 0).sum())
    most_candidates = max(most_candidates, 4 * int(g.state()[1].max()) + 4 * cc.nslots(L))
    assert not bool(cp.overflowed.any()) and cp.capacity == cc.max_points(L) == g.contact_max_points()
  if L > 1:
    assert pair_points > 0 and most_candidates > 64
  g.close()


# ------------------------------------------------------------------------------------------------ 2. capacity and `last`
def test_capacity_and_last(ref_pool, verts):
  from stackrl_amd.contacts import ContactPoints, ROW_WORDS
  L = 8
  g = _mk(ref_pool, L)
  g.reset()
  a = _centre(g)
  for _ in range(4):
    g.step(a)
  full = g.contact_points().cpu()
  e0 = int(full.count.argmax())
  n0 = int(full.count[e0])
  assert n0 >= 2
  for C in (n0 - 1, n0, 1):
    # sentinels in every row, and in a tail behind the last env's rows
    bodies = torch.full((N * C + 3, 2), 77, dtype=torch.int32, device='cuda')
    rows = torch.full((N * C + 3, ROW_WORDS), 7.5, dtype=torch.float32, device='cuda')
    out = ContactPoints(torch.full((N,), -5, dtype=torch.int32, device='cuda'), bodies[:N * C].view(N, C, 2), rows[:N * C].view(N, C, ROW_WORDS))
    got = g.contact_points(out=out)
    assert got.rows.data_ptr() == rows.data_ptr() and got.capacity == C
    assert torch.equal(got.count.cpu(), full.count)                   # the true total, whatever the capacity
    assert bool(got.overflowed[e0]) == (n0 > C)
    for e in range(N):
      n = min(int(full.count[e]), C)
      assert torch.equal(got.bodies[e, :n].cpu(), full.bodies[e, :n])
      assert torch.equal(got.rows[e, :n].cpu().view(torch.int32), full.rows[e, :n].view(torch.int32))
      assert bool((got.bodies[e, n:] == 77).all()) and bool((got.rows[e, n:] == 7.5).all()), (C, e)
    assert bool((bodies[N * C:] == 77).all()) and bool((rows[N * C:] == 7.5).all())
  # `last=True`: the full answer filtered by the last placed body
  last = g.contact_points(last=True).cpu()
  nb = g.state()[1]
  kept = 0
  for e in range(N):
    n = int(full.count[e])
    keep = ((full.bodies[e, :n] == int(nb[e]) - 1).any(-1)).nonzero().flatten()
    assert int(last.count[e]) == len(keep)
    assert torch.equal(last.bodies[e, :len(keep)], full.bodies[e, :n][keep])
    assert torch.equal(last.rows[e, :len(keep)].view(torch.int32), full.rows[e, :n][keep].view(torch.int32))
    kept += len(keep)
  assert 0 < kept < int(full.count.sum())
  _assert_equals_restatement(g, last, verts, 'last', last=True)
  t = full.tuples(e0)
  assert len(t) == n0 and len(t[0]) == 14 and t[0][0] == 0 and t[0][1:5] == (int(full.bodies[e0, 0, 0]), int(full.bodies[e0, 0, 1]), -1, -1)
  assert t[0][5] == tuple(full.position_on_a[e0, 0].tolist()) and t[0][9] == float(full.normal_force[e0, 0])
  g.close()


# ------------------------------------------------------------------------------------------------ 3. other states
def test_no_contact_after_reset_and_after_the_auto_reset(ref_pool):
  L = 2
  g = _mk(ref_pool, L)
  assert int(g.contact_points().count.abs().sum()) == 0          # a handle that has never been reset holds no body
  g.reset()
  assert int(g.contact_points().count.abs().sum()) == 0
  a = _centre(g)
  for _ in range(L):
    _, _, done = g.step(a)
  assert bool(done.all()) and int(g.contact_points().count.min()) > 0
  _, _, done = g.step(a)                                           # the auto-reset call (env.py:235-236)
  assert not bool(done.any()) and int(g.contact_points(wrench=True).count.abs().sum()) == 0
  assert not bool(g.contact_points(wrench=True).wrench.any())
  g.close()


def test_stack_v2_env_counts_bodies_not_list_positions(ref_pool, verts):
  from stackrl_amd import env as envs
  L = 4
  g = envs.make('Stack-v2', n_parallel=N, seed=21, pool=ref_pool, block=True, episode_length=L, orientation_freedom=1,
                ordering_freedom=True, **KW)
  g.reset()
  total = 0
  for t in range(L):
    g.step(g.sample())
    cp = g.contact_points(wrench=True).cpu()
    total += int(_assert_equals_restatement(g, cp, verts, 'v2 step {}'.format(t)).sum())
    assert np.array_equal(cp.count.numpy(), g.contacts()[1])
    assert all(int(cp.bodies[e, :int(cp.count[e])].max()) <= t for e in range(N) if int(cp.count[e]))   # (written rows only)
  assert total > 0
  g.close()


def test_pipelined_env_equals_the_single_handle(ref_pool):
  from stackrl_amd import env as envs
  L = 4
  one = _mk(ref_pool, L, seed=9)
  pipe = _mk(ref_pool, L, seed=9, cls=envs.PipelinedVecStackEnv, groups=2)
  one.reset(), pipe.reset()
  a = _centre(one)
  for t in range(3):
    one.step(a), pipe.step(a)
    for kw in (dict(wrench=True), dict(last=True, capacity=3)):
      x, y = one.contact_points(**kw), pipe.contact_points(**kw)
      assert torch.equal(x.count, y.count) and int(x.count.sum()) > 0
      for e in range(N):
        n = min(int(x.count[e]), x.capacity)
        assert torch.equal(x.bodies[e, :n], y.bodies[e, :n]) and torch.equal(x.rows[e, :n].view(torch.int32), y.rows[e, :n].view(torch.int32))
      if 'wrench' in kw:
        assert torch.equal(x.wrench.view(torch.int32), y.wrench.view(torch.int32))
  one.close(), pipe.close()


# ------------------------------------------------------------------------------------------------ 4. no side effects
def test_a_call_changes_nothing(ref_pool):
  """One handle, the same scripted episode twice from the snapshot of its reset, through the auto-reset: without and with
  `contact_points` calls between the steps.  Observations, rewards, dones and state records are bit-equal."""
  L = 4
  g = _mk(ref_pool, L)
  g.reset()
  snap = g.get_state()
  a = _centre(g)

  def run(calls):
    out = []
    for t in range(L + 2):
      (om, oo), r, d = g.step(a)
      if calls:
        before = g.get_state().records
        g.contact_points(wrench=True), g.contact_points(last=True, capacity=1), g.contact_points(capacity=2)
        assert torch.equal(before, g.get_state().records), t
      out.append((om.clone(), oo.clone(), r.clone().view(torch.int32), d.clone(), g.get_state().records))
    return out
  plain = run(False)
  g.set_state(snap)
  called = run(True)
  for t, (x, y) in enumerate(zip(plain, called)):
    assert all(torch.equal(p, q) for p, q in zip(x, y)), t
  g.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(ref_pool):
  from stackrl_amd import lib as _lib
  from stackrl_amd.config import StackConfig, EINVAL, ENOMESH, OK
  lib = _lib.load()
  L = 2
  g = _mk(ref_pool, L)
  cnt = torch.zeros(N, dtype=torch.int32, device='cuda')
  bod = torch.zeros((N, 4, 2), dtype=torch.int32, device='cuda')
  rows = torch.zeros((N, 4, lib.srl_contact_row_words()), dtype=torch.float32, device='cuda')
  assert lib.srl_contact_row_words() == cc.ROW_WORDS
  P = lambda t: t.data_ptr()

  def refused(code, text, *args):
    assert lib.srl_contact_points(*args) == code
    assert text in lib.srl_last_error().decode(), lib.srl_last_error()
  refused(EINVAL, 'null env', None, 0, 4, P(cnt), P(bod), P(rows), None, None)
  refused(EINVAL, 'null output', g._h, 0, 4, None, P(bod), P(rows), None, None)
  refused(EINVAL, 'null output', g._h, 0, 4, P(cnt), None, P(rows), None, None)
  refused(EINVAL, 'null output', g._h, 0, 4, P(cnt), P(bod), None, None, None)
  refused(EINVAL, 'capacity must be at least 1', g._h, 0, 0, P(cnt), P(bod), P(rows), None, None)
  refused(EINVAL, 'last_only must be 0 or 1', g._h, 2, 4, P(cnt), P(bod), P(rows), None, None)
  refused(EINVAL, 'last_only must be 0 or 1', g._h, -1, 4, P(cnt), P(bod), P(rows), None, None)
  with pytest.raises(ValueError, match='capacity must be at least 1'):
    g.contact_points(capacity=0)
  n = ctypes.c_int32()
  assert lib.srl_contact_max_points(None, ctypes.byref(n)) == EINVAL and 'null env' in lib.srl_last_error().decode()
  assert lib.srl_contact_max_points(g._h, None) == EINVAL and 'null output' in lib.srl_last_error().decode()
  assert lib.srl_contact_max_points(g._h, ctypes.byref(n)) == OK and n.value == 4 * L + 4 * cc.nslots(L)
  # before srl_load_meshes
  c = StackConfig(n_envs=N, episode_length=L, **KW).to_c()
  h = ctypes.c_void_p()
  assert lib.srl_create(ctypes.byref(c), ctypes.byref(h)) == OK
  try:
    refused(ENOMESH, 'srl_load_meshes must be called first', h, 0, 4, P(cnt), P(bod), P(rows), None, None)
  finally:
    lib.srl_destroy(h)
  assert lib.srl_contact_points(g._h, 0, 4, P(cnt), P(bod), P(rows), None, None) == OK      # (the arguments were fine)
  torch.cuda.synchronize()
  g.close()


# ------------------------------------------------------------------------------------------------ 6. momentum balance
def momentum_balance(g, pool):
  """One sub-step on the env as it stands; per body (env, slot): the error of m (v1 - v_free(v0)) = dt * net contact force,
  largest component, and its bound.

  v_free is what the sub-step's first phase (`body_frame`, csrc/settle.hip) makes of v0 before the solver: v * lin_damp, then
  v.z - gravity * dt; nothing after the solver touches the velocities.  The solver adds (d / m) * delta to v once per row and
  application — a warm start and then at most one per sweep — and the manifold's accumulated impulse is the sum of those deltas,
  so the identity holds up to rounding: every application rounds the velocity once (relative 2^-24 of a velocity no larger
  than the largest of |v_free|, |v1|, in momentum m times that) and the accumulated impulse once (relative 2^-24 of an impulse
  no larger than the body's largest); the right side rounds each row's quotient, product and sum once.  Bound: 2^-24 x
  ((sweeps + 1) x 3 rows x points + 3 x points) applications x max(largest impulse, m x largest velocity), times 4 for the
  order of summation."""
  c = g.config
  dt, grav = np.float32(c.sim_time_step), np.float32(c.gravity)
  lin = np.float32((1.0 - float(c.linear_damping)) ** float(c.sim_time_step))
  poses, nb, _, _ = g.state()
  v0 = g.velocities()[:, :, 0:3]
  g.step_simulation(1)
  v1 = g.velocities()[:, :, 0:3].astype(np.float64)
  sweeps = g.sweeps()
  cp = g.contact_points(wrench=True).cpu()
  out = []
  for e in range(g.batch_size):
    n = int(cp.count[e])
    bodies, rows = cp.bodies[e, :n].numpy(), cp.rows[e, :n].numpy().astype(np.float64)
    for b in range(int(nb[e])):
      m = float(pool.mass_com[int(poses[e, b, 7]), 0])
      vf = (v0[e, b] * lin).astype(np.float32)
      vf[2] = vf[2] - grav * dt
      lhs = m * (v1[e, b] - vf.astype(np.float64))
      rhs = float(dt) * cp.wrench[e, b, 0:3].numpy().astype(np.float64)
      mine = (bodies == b).any(-1)
      pts = int(mine.sum())
      assert pts == int(cp.wrench[e, b, 3])
      imax = float(dt) * np.abs(rows[mine][:, [10, 11, 15]]).max() if pts else 0.0
      vmax = max(np.abs(vf).max(), np.abs(v1[e, b]).max())
      bound = 4 * 2.0 ** -24 * ((int(sweeps[e]) + 1) * 3 * pts + 3 * pts + 1) * max(imax, m * vmax)
      out.append((e, b, pts, float(np.abs(lhs - rhs).max()), bound))
  return out


def test_momentum_balance_of_a_sub_step(ref_pool):
  """Largest error / bound observed: see DESIGN.md, "Contact points"."""
  L = 8
  g = _mk(ref_pool, L)
  g.reset()
  a = _centre(g)
  worst, with_pairs = 0.0, 0
  for t in range(5):
    g.step(a)
  for e, b, pts, err, bound in momentum_balance(g, ref_pool):
    print('env {} body {}: {} points, error {:.3e}, bound {:.3e}, ratio {:.3f}'.format(e, b, pts, err, bound, err / bound))
    worst = max(worst, err / bound)
    with_pairs += pts > 0
    assert err <= bound, (e, b, pts, err, bound)
  print('largest error / bound: {:.3f}'.format(worst))
  assert with_pairs >= N
  g.close()
