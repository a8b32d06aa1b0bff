"""The update's glue kernels (csrc/learner.hip: `srl_td_epilogue`, `srl_adam_step`, `srl_gumbel_topk`, `srl_replay_scatter` /
`_gather`, `srl_logit_extrema`) and the two arg-max heads of csrc/qnet.hip at their edges, held to the float64 references and
the cases of tests/learner_cases.py (tests/test_learner_cases.py checks those references and that the cases tell wrong
variants apart, without a GPU).

Every output buffer is NaN- or sentinel-filled before the call: an element a kernel never writes fails its comparison.
Kernels are called through `qops` where `qops` lets the caller own the outputs or is itself what is checked, and through
`qops.load()` (the C ABI) otherwise.  Tolerances: learner_cases.py (exact for integers, indices, bytes and copies;
C 2^-24 scale with C = 4 x the float32 host restatement's error for float32 arithmetic)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import learner_cases as C

pytestmark = pytest.mark.gpu

NAN = float('nan')


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
  return t.detach().cpu().numpy()


def _ptr(t):
  return None if t is None else t.data_ptr()


def _ok(rc, err):
  from stackrl_amd import qops
  assert rc == 0, getattr(qops.load(), err)().decode()


# ================================================================================================ arg-max heads
def _policy(adv, eps=0.0, u=None, rnd=None):
  from stackrl_amd import qops
  B, A = adv.shape
  a = dev(adv)
  u = dev(np.full(B, 0.5, np.float32) if u is None else u)
  rnd = dev(np.zeros(B, np.int64) if rnd is None else rnd)
  out = torch.full((B,), -7, dtype=torch.int64, device='cuda')
  _ok(qops.load().srl_policy_head(a.data_ptr(), u.data_ptr(), rnd.data_ptr(), float(eps), out.data_ptr(), B, A, qops._stream(a)),
      'srl_qnet_last_error')
  return host(out)


def _boltzmann(adv, T, seed=0):
  from stackrl_amd import qops
  B, A = adv.shape
  a = dev(adv)
  keys = torch.randint(0, 2 ** 32, (B, 2), dtype=torch.int64, generator=torch.Generator().manual_seed(seed)).cuda()
  out = torch.full((B,), -7, dtype=torch.int64, device='cuda')
  _ok(qops.load().srl_boltzmann_head(a.data_ptr(), keys.data_ptr(), float(T), out.data_ptr(), B, A, qops._stream(a)),
      'srl_qnet_last_error')
  return host(out)


def test_policy_head_all_minus_inf_row_gives_action_0():
  """`torch.argmax` of an all -inf row is 0.  Until the per-thread start of the reduction could no longer win it, this row
  returned 2147483647 (the start index of a thread that met no entry above -3.0e38), which the env rejects."""
  adv = np.full((3, 2401), -np.inf, np.float32)
  adv[1] = np.random.RandomState(0).normal(size=2401)          # its neighbours are ordinary rows
  got = _policy(adv)
  print('actions', got.tolist())
  assert got.tolist() == C.argmax_ref(adv).tolist() and got[0] == 0 and got[2] == 0


@pytest.mark.parametrize('A', C.HEAD_AS)
def test_policy_head_rows(A):
  """eps = 0: the action is `argmax_ref` on every kind of row — random, with -inf entries, finite below -3e38, nothing but
  -inf (0), a tie (the lowest index), and with NaN entries (skipped; nothing else: 0).  eps = 1 takes the random draw."""
  rows = C.head_rows(A)
  adv = np.stack([r for _, r in rows])
  want = C.argmax_ref(adv)
  got = _policy(adv)
  for (kind, _), g, w in zip(rows, got.tolist(), want.tolist()):
    assert 0 <= g < A and g == w, (kind, g, w)
  rnd = np.arange(len(rows), dtype=np.int64) % A
  assert _policy(adv, eps=1.0, rnd=rnd).tolist() == rnd.tolist()


@pytest.mark.parametrize('A', C.HEAD_AS)
@pytest.mark.parametrize('T', [0.7, 50.0])
def test_boltzmann_head_rows(A, T):
  """Any temperature: an index in [0, A) on every row without NaN (nothing but -inf included), the one finite entry of a row
  that has one; at T = 50 the scores of the row below -3e38 stay finite and the noise is below their rounding: its maximum."""
  rows = [(k, r) for k, r in C.head_rows(A) if 'NaN' not in k]
  adv = np.stack([r for _, r in rows])
  got = _boltzmann(adv, T, seed=A)
  for (kind, r), g in zip(rows, got.tolist()):
    assert 0 <= g < A, (kind, g)
    if kind == 'one finite':
      assert g == (2 * A) // 3
    if kind == 'some -inf':
      assert np.isfinite(r[g])
    if kind == 'below -3e38' and T == 50.0:
      assert g == A // 2


# ================================================================================================ Adam
@pytest.mark.parametrize('betas', C.ADAM_BETAS)
@pytest.mark.parametrize('n', C.ADAM_NS)
def test_adam_step_against_float64(n, betas):
  """p, m, v and the four state floats after each of 6 steps with redrawn gradients, unequal betas included; the buffers sit
  inside longer ones whose NaN margin must survive (the scalar tail stops at n)."""
  from stackrl_amd import qops
  c = C.adam_case(n, betas)
  ref = C.adam_ref(c['p'], c['m'], c['v'], c['grads'], c['lr'], c['b1'], c['b2'], c['eps'])
  sc = C.adam_scales(c, ref)
  pad = 8
  P, M, V = (torch.cat([dev(c[k]), torch.full((pad,), NAN, device='cuda')]) for k in ('p', 'm', 'v'))
  S = torch.tensor([0.0, 1.0, 1.0, 0.0], device='cuda')
  for t in range(C.ADAM_STEPS):
    G = dev(c['grads'][t])
    qops.adam_step(P[:n], G, M[:n], V[:n], S, c['lr'], c['b1'], c['b2'], c['eps'])
    got = dict(p=host(P[:n]), m=host(M[:n]), v=host(V[:n]), state=host(S))
    e = C.adam_errors(got, ref[t], sc[t])
    print('adam n', n, 'betas', betas, 'step', t + 1, 'error / (2^-24 scale)', e,
          'float32 host', {k: C.ADAM_MEASURED[betas][k][t] for k in e}, 'bound', {k: C.ADAM_C[betas][k][t] for k in e})
    assert float(got['state'][0]) == t + 1
    for k in e:
      assert e[k] <= C.ADAM_C[betas][k][t], (k, t + 1, e[k], C.ADAM_C[betas][k][t])
    for X in (P, M, V):
      assert bool(torch.isnan(X[n:]).all())


# ================================================================================================ TD epilogue
def _td_call(c, ws=None, with_grad=True):
  """srl_td_epilogue through the ABI on NaN-filled outputs.  ws: dict(scratch, ticket) the caller keeps."""
  from stackrl_amd import qops
  mb, A = c['mb'], c['A']
  if ws is None:
    ws = {}
  if 'ticket' not in ws:
    ws.update(ticket=torch.zeros(1, dtype=torch.int32, device='cuda'), scratch=torch.full((2 * mb,), NAN, device='cuda'))
  q, qt, act, rew, term = (dev(c[k]) for k in ('q', 'qt', 'actions', 'rewards', 'terminal'))
  qo = dev(c['qo']) if c['double'] else None                   # plain DQN never reads the online net's values
  w = dev(c['weights']) if c['weights'] is not None else None
  out = torch.full((2,), NAN, device='cuda'); td_abs = torch.full((mb,), NAN, device='cuda')
  logits = torch.full((mb,), NAN, device='cuda')
  grad = torch.full((mb, A), NAN, device='cuda') if with_grad else None
  _ok(qops.load().srl_td_epilogue(q.data_ptr(), _ptr(qo), qt.data_ptr(), act.data_ptr(), rew.data_ptr(), term.data_ptr(), _ptr(w),
                                  c['gamma'], -1.0 if c['huber'] is None else c['huber'], c['reward_scale'], int(c['double']),
                                  c['prio_eps'], mb, A, out.data_ptr(), out[1:].data_ptr(), td_abs.data_ptr(),
                                  logits.data_ptr(), _ptr(grad), ws['scratch'].data_ptr(), ws['ticket'].data_ptr(),
                                  qops._stream(q)), 'srl_learner_last_error')
  torch.cuda.synchronize()
  return dict(loss=host(out)[0], mtd=host(out)[1], td_abs=host(td_abs), logits=host(logits),
              grad_q=host(grad) if with_grad else None, ticket=int(ws['ticket'][0]))


def _td_check(c, got, label):
  ref, lo = C.td_ref(c), C.td_f32(c)
  e = C.td_errors(got, ref)
  print('td', label, sorted(c['notes']), 'error / (2^-24 scale)', e, 'float32 host', C.TD_MEASURED, 'bound', C.TD_C)
  assert np.array_equal(got['td_abs'], lo['td_abs'])                  # q - y in float32, in the header's order: exact
  for k in e:
    assert e[k] <= C.TD_C[k], (k, e[k], C.TD_C[k])
  off = np.ones((c['mb'], c['A']), bool); off[np.arange(c['mb']), c['actions']] = False
  assert not np.isnan(got['grad_q']).any() and (got['grad_q'][off] == 0).all()       # dense: exactly zero off the action
  assert got['ticket'] == 0


@pytest.mark.parametrize('case', C.TD_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_td_epilogue_against_float64(case):
  """Loss, mean TD, |TD|, new priorities and the dense d loss / d Q at every shape and switch of TD_CASES, with the designed
  samples of `td_case` (ties inside a thread and between threads, a -inf selecting row, td == 0, |td| == delta, td < -delta,
  both terminal values, the taken action at the arg-max); without grad_q the other outputs are the same bits."""
  c = C.td_case(*case)
  got = _td_call(c)
  _td_check(c, got, case)
  bare = _td_call(c, with_grad=False)
  for k in ('loss', 'mtd', 'td_abs', 'logits'):
    assert np.array_equal(np.asarray(got[k]), np.asarray(bare[k])), k
  assert bare['ticket'] == 0


@pytest.mark.parametrize('mb,A', [(5, 257), (32, 2401)])
def test_td_epilogue_reuses_its_workspace(mb, A):
  """Three calls with different inputs on ONE workspace through `qops.td_epilogue`, each correct, the ticket word 0 after
  each; a fourth repeating the first inputs returns the first call's bits (and those of the call through the ABI)."""
  from stackrl_amd import qops
  ws = {}
  first = None
  cases = [C.td_case(mb, A, *C.TD_SWITCHES[i], seed=i + 1) for i in (0, 2, 1)]
  for i, c in enumerate(cases + cases[:1]):
    loss, mtd, td_abs, logits, grad = qops.td_epilogue(dev(c['q']), dev(c['qo']) if c['double'] else None, dev(c['qt']), dev(c['actions']),
                                                       dev(c['rewards']), dev(c['terminal']).bool(),
                                                       dev(c['weights']) if c['weights'] is not None else None, c['gamma'], c['huber'],
                                                       c['reward_scale'], c['double'], c['prio_eps'], ws)
    got = dict(loss=host(loss), mtd=host(mtd), td_abs=host(td_abs), logits=host(logits), grad_q=host(grad), ticket=int(ws['ticket'][0]))
    _td_check(c, got, ('call', i))
    if i == 0:
      first = got
      abi = _td_call(c)
      for k in ('loss', 'mtd', 'td_abs', 'logits', 'grad_q'):
        assert np.array_equal(np.asarray(got[k]), np.asarray(abi[k])), k
  for k in ('loss', 'mtd', 'td_abs', 'logits', 'grad_q'):
    assert np.array_equal(np.asarray(got[k]), np.asarray(first[k])), k


# ================================================================================================ Gumbel top-k
def _topk(logits, u, alpha_t, k, fill=0x00):
  """srl_gumbel_topk through the ABI: outputs sentinel-filled, the scratch filled with the byte `fill`."""
  from stackrl_amd import qops
  L = qops.load()
  n = len(logits)
  l, uu = dev(logits), dev(u)
  need = int(L.srl_gumbel_topk_scratch_bytes(n, k))
  assert need == -(-n // C.TOPK_CHUNK) * k * 8
  scratch = torch.full((need,), fill, dtype=torch.uint8, device='cuda')
  idx = torch.full((k,), -7, dtype=torch.int64, device='cuda'); key = torch.full((k,), NAN, device='cuda')
  _ok(L.srl_gumbel_topk(l.data_ptr(), uu.data_ptr(), alpha_t.data_ptr(), n, k, idx.data_ptr(), key.data_ptr(), scratch.data_ptr(),
                        need, qops._stream(l)), 'srl_learner_last_error')
  return host(idx), host(key)


def _alpha(a):
  return torch.tensor([a], dtype=torch.float32, device='cuda')


def _topk_check(l, u, a, k, idx, key, label, exact=False):
  ridx, rkey, decided = C.topk_decided(l, u, a, k)
  fin = np.isfinite(rkey)
  assert np.array_equal(np.isfinite(key), fin) and (key[~fin] == -np.inf).all() and (idx[~fin] == 0).all(), label
  assert ((idx >= 0) & (idx < len(l))).all()
  tol = C.TOPK_C * C.U * C.topk_key_scale(l, u, a, ridx)
  err = np.where(fin, np.abs(np.where(fin, key, 0.0).astype(np.float64) - np.where(fin, rkey, 0.0)), 0.0)
  print('top-k', label, 'largest key error / tolerance', float((err / tol).max()), 'decided positions', int(decided.sum()), 'of', k)
  assert (err <= tol).all(), label
  if exact:
    assert np.array_equal(idx, ridx), (label, idx.tolist(), ridx.tolist())
  assert np.array_equal(idx[decided], ridx[decided]), label
  got = idx[fin]
  assert len(set(got.tolist())) == len(got) and np.isfinite(np.asarray(l)[got]).all()    # distinct, sampleable slots only


@pytest.mark.parametrize('placement,n', C.TOPK_DESIGNED)
@pytest.mark.parametrize('k', [8, 32])
def test_gumbel_topk_designed_ties(placement, n, k):
  """Equal keys by construction (lattice logits, one Gumbel term): the indices equal `topk_ref`'s — the lower index first —
  exactly, with the duplicated leaders in one thread's two slots, two threads, two chunks and the ragged last chunk, and, at
  k = 32, runs of equal lattice values behind them."""
  l, u, a = C.topk_designed(n, placement)
  idx, key = _topk(l, u, _alpha(a), k)
  _topk_check(l, u, a, k, idx, key, (placement, n, k), exact=True)


@pytest.mark.parametrize('name,n,k,slots', C.TOPK_PLACEMENTS, ids=lambda x: str(x) if not isinstance(x, tuple) else 'slots')
def test_gumbel_topk_placements(name, n, k, slots):
  """All sampleable slots in one chunk; 3 per chunk with k = 32; fewer than k overall (the finite entries in order, then key
  -inf / index 0); none."""
  l, u, a = C.topk_placement(n, slots)
  idx, key = _topk(l, u, _alpha(a), k)
  _topk_check(l, u, a, k, idx, key, (name, n, k))
  assert int(np.isfinite(key).sum()) == min(k, len(slots))


@pytest.mark.parametrize('n,k', C.TOPK_RANDOM)
def test_gumbel_topk_random(n, k):
  """Random logits (30 % -inf) and uniforms at every n around the chunk size and every k, k > n included: keys within float32
  rounding of the float64 keys, indices equal wherever the float64 gaps exceed it; the scratch's previous contents (0x00 or
  0xFF bytes) change nothing; alpha is read from the device at every call; alpha = 0 returns no -inf slot."""
  l, u, a = C.topk_random(n, k)
  at = _alpha(a)
  idx, key = _topk(l, u, at, k, fill=0x00)
  _topk_check(l, u, a, k, idx, key, (n, k))
  idx2, key2 = _topk(l, u, at, k, fill=0xFF)
  assert np.array_equal(idx, idx2) and np.array_equal(key, key2)
  for a2 in (2.0, 0.0):                                         # rewritten in place: the same device word
    at.fill_(a2)
    idx3, key3 = _topk(l, u, at, k)
    _topk_check(l, u, a2, k, idx3, key3, (n, k, 'alpha', a2))


def test_gumbel_topk_through_qops_follows_alpha_on_one_workspace():
  from stackrl_amd import qops
  n, k = 4097, 8
  l, u, a = C.topk_random(n, k, seed=3)
  ws = {}
  at = _alpha(a)
  ld, ud = dev(l), dev(u)
  for a2 in (a, 2.0, 0.0, a):
    at.fill_(a2)
    idx, key = qops.gumbel_topk(ld, ud, at, k, ws)
    _topk_check(l, u, C.f32s(a2), k, host(idx), host(key), ('qops', a2))
    ref = _topk(l, u, at, k, fill=0xFF)
    assert np.array_equal(host(idx), ref[0]) and np.array_equal(host(key), ref[1])


# ================================================================================================ replay scatter / gather
def _mem_dev(mem):
  return {k: dev(v) for k, v in mem.items()}


def _mem_equal(d, model, label):
  for k in ('m0', 'm1', 'reward', 'terminal', 'action', 'logits'):
    a, b = host(d[k]), model[k]
    assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (label, k)     # bytes: -inf and all


@pytest.mark.parametrize('bytes0,bytes1', C.REPLAY_ROW_BYTES)
@pytest.mark.parametrize('B', C.REPLAY_BS)
@pytest.mark.parametrize('part_len', C.REPLAY_PART_LENS)
def test_replay_scatter_against_the_memory_model(bytes0, bytes1, B, part_len):
  """The whole memory after `qops.replay_scatter` equals `scatter_ref`'s model byte for byte: the written rows, their logit
  -inf, every other row of every tensor untouched — at the first and the last slot of the partitions."""
  from stackrl_amd import qops
  model = C.replay_memory(B, part_len, bytes0, bytes1)
  d = _mem_dev(model)
  for slot in sorted({0, part_len - 1}):
    tr = C.replay_transitions(B, bytes0, bytes1, seed=slot)
    qops.replay_scatter((dev(tr['s0']), dev(tr['s1'])), dev(tr['reward']), dev(tr['terminal']).bool(), dev(tr['action']), slot,
                        part_len, (d['m0'], d['m1']), d['reward'], d['terminal'], d['action'], d['logits'])
    model = C.scatter_ref(model, tr, slot, part_len)
    _mem_equal(d, model, ('slot', slot))


def _gather(d, idx, part_len, n_steps, literal, b0, b1, weights, want_next):
  from stackrl_amd import qops
  mb = len(idx)
  i = dev(idx)
  u8 = lambda *s: torch.full(s, 0xA5, dtype=torch.uint8, device='cuda')
  o = dict(s0=u8(mb, b0), s1=u8(mb, b1), n0=u8(mb, b0), n1=u8(mb, b1), action=torch.full((mb,), -7, dtype=torch.int64, device='cuda'),
           reward=torch.full((mb,), NAN, device='cuda'), terminal=u8(mb),
           weight=torch.full((mb,), NAN, device='cuda') if weights is not None else None,
           next=torch.full((mb,), -7, dtype=torch.int64, device='cuda') if want_next else None)
  sc = [torch.tensor([x], dtype=torch.float32, device='cuda') for x in weights] if weights is not None else [None] * 3
  _ok(qops.load().srl_replay_gather(i.data_ptr(), mb, part_len, n_steps, int(literal), _ptr(o['next']), d['m0'].data_ptr(),
                                    d['m1'].data_ptr(), b0, b1, d['reward'].data_ptr(), d['terminal'].data_ptr(),
                                    d['action'].data_ptr(), d['logits'].data_ptr(), _ptr(sc[0]), _ptr(sc[1]), _ptr(sc[2]),
                                    o['s0'].data_ptr(), o['s1'].data_ptr(), o['n0'].data_ptr(), o['n1'].data_ptr(),
                                    o['action'].data_ptr(), o['reward'].data_ptr(), o['terminal'].data_ptr(), _ptr(o['weight']),
                                    qops._stream(i)), 'srl_learner_last_error')
  return {k: (None if v is None else host(v)) for k, v in o.items()}


@pytest.mark.parametrize('bytes0,bytes1', C.REPLAY_ROW_BYTES)
@pytest.mark.parametrize('B', C.REPLAY_BS)
@pytest.mark.parametrize('part_len', C.REPLAY_PART_LENS)
def test_replay_gather_against_the_memory_model(bytes0, bytes1, B, part_len):
  """Rows, next rows, action, reward and terminal bit-exact and the next-row indices equal `gather_ref`, for both next-row
  formulas and n_steps 1 and 3 through the ABI (the header: the row n_steps on inside the partition; reward and flag of that
  row), with and without weights and next_dev; the importance weight within C 2^-24 (1 + |exponent|), relative.  The memory
  is left as it was."""
  from stackrl_amd import qops
  model = C.replay_memory(B, part_len, bytes0, bytes1)
  d = _mem_dev(model)
  idx = C.gather_indices(B, part_len)
  fin = C.finite_rows(model)
  mn = float(model['logits'][fin].min()) if len(fin) else 0.0
  wa = (C.f32s(C.GATHER_ALPHA), C.f32s(C.GATHER_BETA), mn)
  worst = 0.0
  for literal in (False, True):
    for n_steps in C.REPLAY_N_STEPS:
      ref = C.gather_ref(model, idx, part_len, n_steps, literal, *wa)
      assert ((ref['next'] >= 0) & (ref['next'] < B * part_len)).all()
      for weights, want_next in ((wa, True), (None, False)):
        got = _gather(d, idx, part_len, n_steps, literal, bytes0, bytes1, weights, want_next)
        for k in ('s0', 's1', 'n0', 'n1', 'action', 'terminal'):
          assert np.array_equal(got[k], ref[k]), (k, literal, n_steps)
        assert np.array_equal(got['reward'].view(np.uint32), ref['reward'].view(np.uint32))
        if want_next:
          assert np.array_equal(got['next'], ref['next'])
        if weights is not None:
          w = got['weight'].astype(np.float64); ok = np.isfinite(ref['weight'])
          assert np.array_equal(w[~ok], ref['weight'][~ok])                  # a -inf logit: exp(+inf)
          rel = np.abs(w[ok] / ref['weight'][ok] - 1) / (C.U * (1 + np.abs(ref['weight_arg'][ok])))
          worst = max(worst, float(rel.max()) if len(rel) else 0.0)
  print('importance weight: largest relative error / (2^-24 (1 + |exponent|))', worst, 'float32 host', C.WEIGHT_MEASURED,
        'bound', C.WEIGHT_C)
  assert worst <= C.WEIGHT_C
  _mem_equal(d, model, 'after the gathers')
  # and `qops.replay_gather` (no next_dev) returns the same minibatch
  m2 = (d['m0'], d['m1'])
  at, bt, mt = (torch.tensor(x, dtype=torch.float32, device='cuda') for x in wa)
  (s, act, rew, nx, term), w = qops.replay_gather(dev(idx), part_len, 1, True, m2, d['reward'], d['terminal'].bool(), d['action'],
                                                  d['logits'], at, bt, mt)
  ref = C.gather_ref(model, idx, part_len, 1, True, *wa)
  assert all(np.array_equal(host(a), ref[k]) for a, k in zip(s + nx, ('s0', 's1', 'n0', 'n1')))
  assert np.array_equal(host(act), ref['action']) and np.array_equal(host(rew), ref['reward'])
  assert np.array_equal(host(term), ref['terminal'] != 0)


# ================================================================================================ logit extrema
def _extrema(x, scratch):
  from stackrl_amd import qops
  t = dev(x)
  v = torch.full((2,), NAN, device='cuda'); i = torch.full((2,), -7, dtype=torch.int64, device='cuda')
  _ok(qops.load().srl_logit_extrema(t.data_ptr(), len(x), v.data_ptr(), i.data_ptr(), scratch.data_ptr(), qops._stream(t)),
      'srl_learner_last_error')
  return float(v[0]), int(i[0]), float(v[1]), int(i[1])


@pytest.mark.parametrize('n', C.EXTREMA_NS)
def test_logit_extrema_against_the_reference(n):
  """Max logit and min FINITE logit with their lowest indices, exactly, at n around the block size and the block cap: ties,
  -inf rows, nothing finite (+inf, 0), a +inf entry (the maximum, never the minimum), a tie seen first by two workgroups."""
  from stackrl_amd import qops
  scratch = torch.full((int(qops.load().srl_logit_extrema_scratch_bytes()),), 0xFF, dtype=torch.uint8, device='cuda')
  for name, x in C.extrema_cases(n):
    got, want = _extrema(x, scratch), C.extrema_ref(x)
    assert got == want, (name, n, got, want)
    (mv, mi), (nv, ni) = qops.logit_extrema(dev(x), {})
    assert (float(mv), int(mi), float(nv), int(ni)) == want, (name, n)
