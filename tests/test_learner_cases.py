"""The references and cases of tests/learner_cases.py, without a GPU.

  * The references are right: `td_ref` against oracle/dqn_oracle.py::dqn_targets, `scatter_ref` / `gather_ref` / `extrema_ref`
    against `RefMemory` and against `stackrl_amd.memory.ReplayMemory` on the CPU (the library formulation) over a sequence of
    adds, samples and priority updates that wraps the partitions, `adam_ref` against `KerasAdam`'s CPU path.
  * The cases have teeth: a numpy restatement of each WRONG variant a kernel could be differs from the reference on the
    cases' own inputs by at least 10 x the tolerance tests/test_learner_kernels_gpu.py applies (in one element at least for
    exact outputs) — this stands in for building wrong kernels.
  * The case lists reach the edges (sizes around the block, chunk and grid limits, every switch, every designed sample).
  * The recorded float32-against-float64 figures behind the tolerances are what `measure_*` measures."""
import math

import numpy as np
import pytest

import learner_cases as C

torch = pytest.importorskip('torch')


# ================================================================================================ recorded figures
def _held(measured, recorded, what):
  assert 0.9 * recorded <= measured <= recorded, (what, measured, recorded)


def test_recorded_figures_are_the_measured_ones():
  for betas, d in C.measure_adam().items():
    for k, per_step in d.items():
      for t, m in enumerate(per_step):
        _held(m, C.ADAM_MEASURED[betas][k][t], ('adam', betas, k, t + 1))
        assert C.ADAM_C[betas][k][t] == 4.0 * C.ADAM_MEASURED[betas][k][t]
  for k, m in C.measure_td().items():
    _held(m, C.TD_MEASURED[k], ('td', k))
    assert C.TD_C[k] == 4.0 * C.TD_MEASURED[k]
  _held(C.measure_topk(), C.TOPK_MEASURED, 'top-k keys'); assert C.TOPK_C == 4.0 * C.TOPK_MEASURED
  _held(C.measure_weight(), C.WEIGHT_MEASURED, 'importance weight'); assert C.WEIGHT_C == 4.0 * C.WEIGHT_MEASURED


# ================================================================================================ references are right
@pytest.mark.parametrize('case', [c for c in C.TD_CASES if c[5] == 0.0], ids=str)
def test_td_ref_equals_the_oracle(case):
  from oracle import dqn_oracle as O
  c = C.td_case(*case)
  r = C.td_ref(c)
  loss, mtd, ad = O.dqn_targets(c['q'], c['qo'], c['qt'], c['actions'], c['rewards'], c['terminal'] != 0, c['gamma'],
                                double=c['double'], huber_delta=c['huber'], weights=c['weights'])
  assert abs(loss - r['loss']) <= 1e-12 * max(1.0, abs(loss)) and abs(mtd - r['mtd']) <= 1e-12
  np.testing.assert_allclose(r['td_abs'], ad, rtol=0, atol=1e-12)
  np.testing.assert_allclose(r['logits'], np.log(ad + c['prio_eps']), rtol=0, atol=1e-9)
  # the gradient is the derivative of the oracle's loss: central differences in float64 at the taken actions (away from the kink)
  h = 1e-6
  for j in range(c['mb']):
    if c['huber'] is not None and abs(abs(r['td'][j]) - c['huber']) < 1e-3:
      continue
    q2 = c['q'].astype(np.float64)
    d = []
    for s in (h, -h):
      q3 = q2.copy(); q3[j, c['actions'][j]] += s
      d.append(O.dqn_targets(q3, c['qo'], c['qt'], c['actions'], c['rewards'], c['terminal'] != 0, c['gamma'], double=c['double'],
                             huber_delta=c['huber'], weights=c['weights'])[0])
    assert abs((d[0] - d[1]) / (2 * h) - r['grad_q'][j, c['actions'][j]]) <= 1e-6
  assert int((r['grad_q'] != 0).sum()) <= c['mb']


def test_argmax_ref():
  x = np.array([[1, 3, 3, -np.inf], [-np.inf] * 4, [np.nan, -np.inf, -5, np.nan], [np.nan] * 4, [-np.inf, -3.3e38, -3.2e38, -np.inf]])
  assert C.argmax_ref(x).tolist() == [1, 0, 2, 0, 2]
  t = torch.tensor(x[:2])
  assert C.argmax_ref(x[:2]).tolist() == t.argmax(-1).tolist()


@pytest.mark.parametrize('literal', [False, True])
def test_memory_refs_equal_the_oracle_and_the_library_formulation(literal):
  """`scatter_ref`, `gather_ref` and `extrema_ref` beside `RefMemory` and `ReplayMemory` on the CPU: 6 partitions of 5 slots,
  13 adds (the partitions wrap twice), samples with weights and priority updates in between."""
  from oracle import dqn_oracle as O
  from stackrl_amd.memory import ReplayMemory
  B, L, mb, alpha, beta = 6, 5, 8, 0.6, 0.7
  b0, b1 = 32, 16
  spec = (((B, 4, 4, 2), torch.uint8), ((B, 16), torch.uint8))
  lib = ReplayMemory(spec, B * L, alpha=alpha, beta=beta, seed=11, device='cpu', reference_next_index=literal)
  assert not lib._fused
  orc = O.RefMemory(B, B * L, literal_next_index=literal)

  def model_of(lib):
    return dict(m0=lib._states[0].numpy().reshape(B * L, b0).copy(), m1=lib._states[1].numpy().reshape(B * L, b1).copy(),
                reward=lib._rewards.numpy().copy(), terminal=lib._terminal.numpy().astype(np.uint8), action=lib._actions.numpy().copy(),
                logits=lib._logits.numpy().copy())
  rng = np.random.RandomState(3)
  model = model_of(lib)
  for t in range(13):
    tr = C.replay_transitions(B, b0, b1, seed=t)
    tr['terminal'] = (rng.rand(B) < 0.2).astype(np.uint8)
    slot = t % L
    lib.add((torch.from_numpy(tr['s0'].reshape(B, 4, 4, 2)), torch.from_numpy(tr['s1'])), torch.from_numpy(tr['reward']),
            torch.from_numpy(tr['terminal'] != 0), torch.from_numpy(tr['action']))
    orc.add([(tr['s0'][i], tr['s1'][i]) for i in range(B)], tr['reward'], tr['terminal'] != 0, tr['action'])
    model = C.scatter_ref(model, tr, slot, L)
    after = model_of(lib)
    for k in ('m0', 'm1', 'reward', 'terminal', 'action'):
      assert np.array_equal(model[k], after[k]), (t, k)
    back = np.arange(B) * L + (t - 1) % L                      # `add` then opens the predecessors: not the scatter's business
    rest = np.setdiff1d(np.arange(B * L), back)
    assert np.array_equal(model['logits'][rest], after['logits'][rest]) and np.isneginf(model['logits'][np.arange(B) * L + slot]).all()
    model['logits'] = after['logits']
    np.testing.assert_allclose(model['logits'], np.array(orc.logits, np.float32), rtol=1e-6)
    mx, imx, mn, imn = C.extrema_ref(model['logits'])
    i, v = lib._argmax_all(); assert (float(v), int(i)) == (mx, imx)
    i, v = lib._argmin_finite(); assert (float(v), int(i) if math.isfinite(mn) else 0) == (mn, imn)
    lg = np.array(orc.logits)
    assert orc._argmax() == imx
    if np.isfinite(lg).any():
      assert orc._argmin_finite() == imn
    if t in (6, 9, 12):
      idx, w, (s, a, r, nx, term) = lib.sample(mb if t == 12 else 4, get_weights=True)
      ii = idx.numpy()
      ref = C.gather_ref(model, ii, L, 1, literal, alpha, beta, float(lib._min_logit))
      assert np.array_equal(ref['next'], lib.next_indexes(idx, 1).numpy())
      assert np.array_equal(s[0].numpy().reshape(len(ii), b0), ref['s0']) and np.array_equal(s[1].numpy(), ref['s1'])
      assert np.array_equal(nx[0].numpy().reshape(len(ii), b0), ref['n0']) and np.array_equal(nx[1].numpy(), ref['n1'])
      assert np.array_equal(a.numpy(), ref['action']) and np.array_equal(r.numpy(), ref['reward'])
      assert np.array_equal(term.numpy(), ref['terminal'] != 0)
      np.testing.assert_allclose(w.numpy(), ref['weight'], rtol=C.WEIGHT_C * C.U * (1 + np.abs(ref['weight_arg']).max()))
      for j, i in enumerate(ii.tolist()):
        s0, a0, r0, s1, t1 = orc.transition(i)
        assert orc.next_index(i, 1) == ref['next'][j]
        assert np.array_equal(s0[0], ref['s0'][j]) and np.array_equal(s1[1], ref['n1'][j]) and a0 == ref['action'][j]
        assert np.float32(r0) == ref['reward'][j] and t1 == bool(ref['terminal'][j])
        assert abs(orc.weight(i, alpha, beta) - ref['weight'][j]) <= 1e-5 * ref['weight'][j]
      if t != 12:
        d = (rng.rand(len(ii)) * 2).astype(np.float32)
        lib.update_priorities(idx, torch.from_numpy(d)); orc.update_priorities(ii.tolist(), d.tolist())
        model['logits'] = lib._logits.numpy().copy()
  assert lib._insert_index == 13 and 13 > 2 * L


@pytest.mark.parametrize('betas', C.ADAM_BETAS)
def test_adam_ref_equals_keras_adam_on_the_cpu(betas):
  """`KerasAdam`'s CPU path is float32 torch: it meets the float64 reference within the bounds the kernel gets."""
  from stackrl_amd.dqn import KerasAdam
  n = 1027
  c = C.adam_case(n, betas)
  ref = C.adam_ref(c['p'], c['m'], c['v'], c['grads'], c['lr'], c['b1'], c['b2'], c['eps'])
  sc = C.adam_scales(c, ref)
  par = torch.nn.Parameter(torch.from_numpy(c['p'].copy()))
  opt = KerasAdam([par], c['lr'], (c['b1'], c['b2']), c['eps'])
  for t in range(C.ADAM_STEPS):
    g = torch.zeros(opt.flat.numel()); g[:n] = torch.from_numpy(c['grads'][t])
    opt.step(g)
    got = dict(p=par.detach().numpy(), m=opt.m[:n].numpy(), v=opt.v[:n].numpy(), state=opt.state.numpy())
    e = C.adam_errors(got, ref[t], sc[t])
    for k in e:
      assert e[k] <= C.ADAM_C[betas][k][t], (k, t + 1, e[k])


def test_topk_ref():
  keys = np.array([0.5, 2.0, -np.inf, 2.0, 1.0])
  idx, key = C.topk_ref(keys, 7)
  assert idx.tolist() == [1, 3, 4, 0, 0, 0, 0] and key[:4].tolist() == [2.0, 2.0, 1.0, 0.5] and np.isneginf(key[4:]).all()
  l, u, a = C.topk_random(4097, 32)
  tv, ti = torch.topk(torch.from_numpy(C.gumbel_keys(l, u, a)), 32)
  assert np.array_equal(C.topk_ref((l, u, a), 32)[0], ti.numpy())


# ================================================================================================ cases have teeth
def _adam_all(variant):
  for betas in C.ADAM_BETAS:
    for n in C.ADAM_NS:
      c = C.adam_case(n, betas)
      args = (c['p'], c['m'], c['v'], c['grads'], c['lr'], c['b1'], c['b2'], c['eps'])
      ref = C.adam_ref(*args)
      yield betas, n, ref, C.adam_ref(*args, variant=variant), C.adam_scales(c, ref)


@pytest.mark.parametrize('variant', ['betas swapped', 'eps after the bias correction', 'eps inside the square root'])
def test_adam_cases_tell_wrong_variants_apart(variant):
  """After the last step.  The swap: in m and v as well as p, at EVERY size, down to one element (one step from zero state
  would not do: the step is lr sign(g) either way).  The two placements of eps show in p where sqrt(v) is near eps: at the
  sizes that hold such a band (1,023 elements and more), for both beta pairs."""
  for betas, n, ref, bad, sc in _adam_all(variant):
    if (betas[0] == betas[1] or n < 3) if variant == 'betas swapped' else n < 1023:
      continue
    t = C.ADAM_STEPS - 1
    e = C.adam_errors(bad[t], ref[t], sc[t])
    for k in (('p', 'm', 'v') if variant == 'betas swapped' else ('p',)):
      assert e[k] >= 10 * C.ADAM_C[betas][k][t], (variant, betas, n, k, e[k], C.ADAM_C[betas][k][t])
  if variant == 'betas swapped':                                # the remark above, held
    c = C.adam_case(1027, (0.9, 0.999))
    args = (c['p'], c['m'], c['v'], c['grads'][:1], c['lr'], c['b1'], c['b2'], 0.0)
    a, b = C.adam_ref(*args)[0]['p'], C.adam_ref(*args, variant=variant)[0]['p']
    assert np.abs(a - b).max() <= 1e-12


TD_VARIANTS = {'Huber gradient without its sign': lambda c: c[3] is not None,
               'terminal ignored': lambda c: True,
               'reward_scale on the whole target': lambda c: c[5] != 0.0,
               'arg-max from the wrong network': lambda c: c[2],
               'ties to the highest index': lambda c: c[2]}


@pytest.mark.parametrize('variant', sorted(TD_VARIANTS))
def test_td_cases_tell_wrong_variants_apart(variant):
  """In |td| or in the gradient, by 10 x the bound at one sample at least, on every case the variant applies to that has room
  for the designed samples (3 samples, 4 actions)."""
  n = 0
  for case in C.TD_CASES:
    if not TD_VARIANTS[variant](case) or case[0] < 3 or case[1] < 4:
      continue
    c = C.td_case(*case)
    ref, bad = C.td_ref(c), C.td_ref(c, variant=variant)
    sc = C.td_scales(ref)
    e_td = np.abs(bad['td_abs'] - ref['td_abs']) / (C.U * sc['td'])
    e_g = np.abs(bad['grad_q'] - ref['grad_q']).max(axis=1) / (C.U * sc['grad'])
    assert e_td.max() >= 10 * C.TD_C['td'] or e_g.max() >= 10 * C.TD_C['grad'], (variant, case)
    n += 1
  assert n >= 3, variant


def test_gather_cases_tell_wrong_variants_apart():
  wa = (C.f32s(C.GATHER_ALPHA), C.f32s(C.GATHER_BETA))
  for B in C.REPLAY_BS:
    L = 9
    mem = C.replay_memory(B, L, 16, 16)
    idx = C.gather_indices(B, L)
    fin = C.finite_rows(mem); mn = float(mem['logits'][fin].min())
    for n_steps in C.REPLAY_N_STEPS:
      for literal in (False, True):
        ref = C.gather_ref(mem, idx, L, n_steps, literal, *wa, mn)
        # importance weight read from the next row's logit
        bad = np.exp(wa[1] * wa[0] * (mn - mem['logits'][ref['next']].astype(np.float64)))
        ok = np.isfinite(ref['weight']) & np.isfinite(bad)
        with np.errstate(invalid='ignore'):
          rel = np.abs(bad / ref['weight'] - 1) / (C.U * (1 + np.abs(ref['weight_arg'])))
        assert (ok & (rel >= 10 * C.WEIGHT_C)).any() or (np.isfinite(ref['weight']) != np.isfinite(bad)).any()
        # the two next-row formulas exchanged: apart wherever there is more than one partition
        other = C.gather_ref(mem, idx, L, n_steps, not literal)
        if B > 1:
          assert (other['next'] != ref['next']).any() and (other['n0'] != ref['n0']).any() and (other['n1'] != ref['n1']).any()
          assert (other['reward'] != ref['reward']).any()
        else:
          assert np.array_equal(other['next'], ref['next'])


def test_topk_cases_tell_wrong_variants_apart():
  for placement, n in C.TOPK_DESIGNED:                        # ties to the HIGHER index
    l, u, a = C.topk_designed(n, placement)
    keys = C.gumbel_keys(l, u, a)
    for k in (8, 32):
      bad = np.lexsort((-np.arange(n), -keys))[:k]
      assert (bad != C.topk_ref(keys, k)[0]).any()
      # and float32 keeps the designed order: equal logits give equal keys, unequal ones stay apart
      k32 = C.gumbel_keys(l, u, a, np.float32).astype(np.float64)
      assert np.array_equal(C.topk_ref(k32, k)[0], C.topk_ref(keys, k)[0])
  m = 0
  for n, k in C.TOPK_RANDOM:                                  # -inf logits not excluded at alpha = 0
    if k < 32 or n < 2047:
      continue
    l, u, _ = C.topk_random(n, k)
    with np.errstate(invalid='ignore'):
      bad = np.lexsort((np.arange(n), np.log(-np.log(u.astype(np.float64)))))[:k]     # every slot's key is its Gumbel term
    assert np.isneginf(l[bad]).any() and (bad != C.topk_ref((l, u, 0.0), k)[0]).any()
    m += 1
  assert m >= 4


def test_extrema_cases_tell_wrong_variants_apart():
  for n in C.EXTREMA_NS:                                      # min taken over non-finite entries
    hit = False
    for name, x in C.extrema_cases(n):
      mx, imx, mn, imn = C.extrema_ref(x)
      if np.isneginf(x).any() and np.isfinite(x).any():
        assert (float(x.min()), int(np.argmin(x))) != (mn, imn)
        hit = True
      if name == '+inf':
        assert mx == np.inf and imx == n // 2 and (n < 2 or (mn == -3.0 and imn == 0) or mn < -3.0)
    assert hit or n < 5


# ================================================================================================ the lists reach the edges
def test_adam_cases_reach_the_edges():
  assert (0.9, 0.999) in C.ADAM_BETAS and any(a == b for a, b in C.ADAM_BETAS) and C.ADAM_STEPS >= 5       # DQN's default; the old case
  ns = C.ADAM_NS
  groups = lambda n: n // 4 + 1                                # one lane per vector group and one for the tail
  assert any(n < 4 and n == 1 for n in ns) and any(n < 4 and n > 1 for n in ns) and any(n % 4 == 0 for n in ns)
  assert any(groups(n) == 256 and n % 4 == 3 for n in ns) and any(groups(n) == 257 and n % 4 == 0 for n in ns)
  assert any(groups(n) > 256 and n % 4 == 3 for n in ns)
  c = C.adam_case(1027, (0.9, 0.999))
  g = np.abs(np.stack(c['grads']))
  assert g.min() < 1e-7 < 1e-6 < g.max() and g.max() > 1.0 and np.abs(c['p']).max() < 1e-2
  assert ((np.sqrt(1e-3) * g > 1e-8) & (np.sqrt(1e-3) * g < 1e-6)).mean() > 0.05          # the band with sqrt(v) near eps
  assert all(not np.array_equal(c['grads'][0], x) for x in c['grads'][1:])


def test_td_cases_reach_the_edges():
  assert set(C.TD_SHAPES) >= {(1, 1), (3, 5), (5, 255), (5, 256), (5, 257), (33, 625), (32, 2401), (32, 9409)}
  assert {(c[0], c[1]) for c in C.TD_CASES} == set(C.TD_SHAPES) and len(set(C.TD_CASES)) == len(C.TD_CASES)
  for small in (True, False):                                 # every switch, both values, at a small and at a product A
    cs = [c for c in C.TD_CASES if (c[1] <= 5) == small and (small or c[1] in (625, 2401, 9409))]
    assert {c[2] for c in cs} == {True, False} and {c[3] is None for c in cs} == {True, False}
    assert {c[4] for c in cs} == {True, False} and {c[5] != 0.0 for c in cs} == {True, False}
  notes = set()
  for case in C.TD_CASES:
    c = C.td_case(*case)
    notes |= {(n, c['double']) for n in c['notes']}
    lo = C.td_f32(c)
    d = np.float32(1.0 if c['huber'] is None else c['huber'])
    if 'td == 0' in c['notes']:
      assert lo['td'][0] == 0.0 and not c['terminal'][0]
    if '|td| == delta' in c['notes']:
      assert lo['td'][1] == d and c['terminal'][1]
    if 'td < -delta' in c['notes']:
      assert lo['td'][2] < -d
    if '-inf row' in c['notes']:
      sel = c['qo'] if c['double'] else c['qt']
      assert np.isneginf(sel[2, :-1]).all() and np.isfinite(sel[2, -1]) and lo['astar'][2] == c['A'] - 1 and np.isfinite(lo['td'][2])
    if 'tie between threads' in c['notes']:
      assert lo['astar'][0] == 1
    if 'tie inside a thread' in c['notes']:
      assert lo['astar'][1] == 2 and (258 - 2) % 256 == 0
    if 'action == arg-max' in c['notes']:
      assert c['actions'][3] == lo['astar'][3]
    if c['mb'] > 1:
      assert set(c['terminal'].tolist()) == {0, 1}
    assert np.isfinite(lo['td_abs']).all() and np.isfinite(lo['logits']).all()
  for n in ('tie between threads', 'tie inside a thread', '-inf row'):
    assert (n, True) in notes and (n, False) in notes
  assert {n for n, _ in notes} >= {'td == 0', '|td| == delta', 'td < -delta', 'action == arg-max'}
  assert any(c[0] % 2 == 1 and c[0] > 32 for c in C.TD_CASES)


def test_topk_cases_reach_the_edges():
  ch = C.TOPK_CHUNK
  assert set(C.TOPK_NS) >= {1, 5, ch - 1, ch, ch + 1, 2 * ch + 1, 40000} and set(C.TOPK_KS) == {1, 8, 32}
  assert any(k > n for n, k in C.TOPK_RANDOM) and set(C.TOPK_RANDOM) == {(n, k) for n in C.TOPK_NS for k in C.TOPK_KS}
  assert {p for p, _ in C.TOPK_DESIGNED} == {'same thread', 'two threads', 'two chunks', 'ragged chunk'}
  for placement, n in C.TOPK_DESIGNED:
    l, u, a = C.topk_designed(n, placement)
    lead = np.flatnonzero(l == 8.0)
    assert len(lead) == 2 and np.all(l * 8 == np.round(l * 8)) and len(set(u.tolist())) == 1 and a == 1.0
    i, j = lead.tolist()
    if placement == 'same thread':
      assert i // ch == j // ch and (j - i) % 256 == 0
    elif placement == 'two threads':
      assert i // ch == j // ch and (j - i) % 256 != 0
    elif placement == 'two chunks':
      assert i // ch != j // ch
    else:
      assert i // ch == j // ch == (n - 1) // ch and n % ch != 0
  names = {p[0] for p in C.TOPK_PLACEMENTS}
  assert names >= {'first chunk', 'middle chunk', 'last chunk', '3 per chunk', 'fewer than k', 'none'}
  for name, n, k, slots in C.TOPK_PLACEMENTS:
    chunks = {s // ch for s in slots}
    assert all(0 <= s < n for s in slots) and len(set(slots)) == len(slots)
    if name in ('first chunk', 'middle chunk', 'last chunk'):
      assert len(chunks) == 1 and len(slots) >= k and chunks == {{'first chunk': 0, 'middle chunk': 10, 'last chunk': (n - 1) // ch}[name]}
    if name.startswith('3 per chunk'):
      assert len(chunks) >= 16 and k == 32 and len(slots) >= k and max(sum(1 for s in slots if s // ch == c) for c in chunks) == 3
    if name == 'fewer than k':
      assert 0 < len(slots) < k


def test_topk_random_inputs_decide_most_positions():
  """The random cases compare indices only where the float64 gaps exceed the keys' float32 rounding: at least 90 % of the
  returned positions of every case, at every alpha the GPU test sets."""
  for n, k in C.TOPK_RANDOM:
    l, u, a = C.topk_random(n, k)
    for alpha in (a, 2.0, 0.0):
      _, _, decided = C.topk_decided(l, u, alpha, k)
      assert decided.mean() >= 0.9, (n, k, alpha, decided.mean())
  for name, n, k, slots in C.TOPK_PLACEMENTS:
    l, u, a = C.topk_placement(n, slots)
    assert C.topk_decided(l, u, a, k)[2].mean() >= 0.9, name


def test_replay_cases_reach_the_edges():
  vec = [(a + b) // 16 for a, b in C.REPLAY_ROW_BYTES]
  assert all(a % 16 == 0 and b % 16 == 0 for a, b in C.REPLAY_ROW_BYTES)
  assert any(v > C.SCATTER_GRID_CAP * 256 for v in vec) and any(2 * v > C.GATHER_GRID_CAP * 256 for v in vec)     # a second trip
  assert any(v < 256 for v in vec) and any(256 < v <= C.SCATTER_GRID_CAP * 256 for v in vec)
  assert 1 in C.REPLAY_BS and max(C.REPLAY_BS) > 1 and 1 in C.REPLAY_PART_LENS and set(C.REPLAY_N_STEPS) == {1, 3}
  for B in C.REPLAY_BS:
    for L in C.REPLAY_PART_LENS:
      idx = C.gather_indices(B, L).tolist()
      assert L - 1 in idx and B * L - 1 in idx and 0 in idx and (B - 1) * L in idx and len(set(idx)) < len(idx)
      assert all(0 <= i < B * L for i in idx)
      for n_steps in C.REPLAY_N_STEPS:
        for literal in (False, True):
          nx = C.next_rows(idx, L, n_steps, literal)
          assert ((nx >= 0) & (nx < B * L)).all()
      mem = C.replay_memory(B, L, 16, 16)
      assert mem['m0'].any() and mem['m1'].any() and mem['reward'].all()         # nothing the scatter could restore by writing zeros


def test_extrema_and_head_cases_reach_the_edges():
  b, cap = C.EXTREMA_BLOCK, C.EXTREMA_MAX_BLOCKS * C.EXTREMA_PER_BLOCK
  assert set(C.EXTREMA_NS) >= {1, b - 1, b, b + 1, cap, cap + 1} and cap == 262144
  assert set(C.EXTREMA_NS) >= {5, 1024, 65536, 300001}                    # the earlier test's sizes stay
  for n in C.EXTREMA_NS:
    cases = dict(C.extrema_cases(n))
    assert {'ties and -inf', 'all -inf', '+inf'} <= set(cases)
    assert np.isposinf(cases['+inf']).sum() == 1
    if n > 2 * b:
      x = cases['tie across blocks']
      i, j = np.flatnonzero(x == 6.0).tolist()
      nblk = min(-(-n // C.EXTREMA_PER_BLOCK), C.EXTREMA_MAX_BLOCKS)
      assert x.max() == 6.0 and ((i // b) % nblk != (j // b) % nblk or nblk == 1)
  assert any(min(-(-n // C.EXTREMA_PER_BLOCK), C.EXTREMA_MAX_BLOCKS) > 1 for n in C.EXTREMA_NS)
  assert set(C.HEAD_AS) == {1, 5, 255, 257, 2401}
  for A in C.HEAD_AS:
    rows = dict(C.head_rows(A))
    assert set(rows) == set(C.HEAD_ROW_KINDS) - (set() if A >= 2 else {'tie', 'NaN and finite', 'NaN and -inf'})
    assert np.isneginf(rows['all -inf']).all() and np.isfinite(rows['one finite']).sum() == 1
    r = rows['below -3e38']; assert np.isfinite(r).any() and r.max() < -3.0e38 and C.argmax_ref(r) == A // 2
    assert np.isneginf(rows['some -inf']).any() or A == 1
