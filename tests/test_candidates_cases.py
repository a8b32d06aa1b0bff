"""CPU tests of the definition of include/stackrl_candidates.h as tests/candidates_cases.py restates it: at radius 0 the
restatement is `lookahead.candidates`; at a radius it has the two properties of a greedy non-maximum suppression and the closed
forms; `candidates.select_reference` (and `select` on CPU tensors) equals it on every case of the GPU test; and
`LookaheadPolicy(radius=...)` calls what it should, with a stand-in evaluator."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import candidates_cases as cases  # noqa: E402
from stackrl_amd import lookahead as la  # noqa: E402

KINDS = ('random', 'quantised', 'neginf', 'nan', 'constant', 'close', 'edge')


def _before(v, i, j):
  """Entry i ranks before entry j (point 1 of the definition, written out)."""
  ni, nj = np.isnan(v[i]), np.isnan(v[j])
  if ni != nj:
    return bool(ni)
  if not ni and v[i] != v[j]:
    return bool(v[i] > v[j])
  return i < j


def test_the_order_is_the_stable_descending_sort():
  for kind, dtype in itertools.product(KINDS, ('float32', 'float64')):
    v = cases.make_values(kind, 2, 2, 7, dtype, 5)
    for b in range(2):
      ranked = cases.order(v[b])
      assert ranked.tolist() == torch.sort(torch.as_tensor(v[b]), descending=True, stable=True).indices.tolist(), (kind, dtype)
      assert all(_before(v[b], int(i), int(j)) for i, j in zip(ranked[:-1], ranked[1:])), (kind, dtype)


@pytest.mark.parametrize('k', (1, 2, 8, 32))
def test_radius_0_is_lookahead_candidates(k):
  for kind, dtype, (G, n_valid), where in itertools.product(KINDS, ('float32', 'float64'), ((1, 1), (3, 2), (3, 3)),
                                                            ('random', 'beyond')):
    if where == 'beyond' and n_valid == G:
      continue
    B, OH = 4, 6
    v = cases.make_values(kind, B, G, OH, dtype, 7 + k)
    a = cases.make_action(where, B, G, OH, n_valid, k)
    want = la.candidates(torch.as_tensor(a), torch.as_tensor(v), k, n_valid, OH * OH)
    cand, count = cases.reference(v, a, k, 0, n_valid, OH)
    assert np.array_equal(cand, want.numpy()), (kind, dtype, G, n_valid, where)
    assert count.tolist() == [k] * B


def _check_properties(case, v, a, cand, count):
  A, N = case.OH * case.OH, case.n_valid * case.OH * case.OH
  r = case.radius
  for b in range(case.B):
    n = int(count[b])
    chosen = [int(c) for c in cand[b, :n]]
    assert 1 <= n <= case.k and cand[b, n:].tolist() == [chosen[0]] * (case.k - n), case.name
    assert chosen[0] == (int(np.clip(a[b], 0, case.G * A - 1)) if a is not None else int(cases.order(v[b, :N])[0])), case.name
    assert all(0 <= c < N for c in chosen[1:]) and len(set(chosen)) == n, case.name
    g, y, x = (np.array(chosen) // A, np.array(chosen) % A // case.OH, np.array(chosen) % case.OH)
    # no two chosen entries of one map lie within the radius
    for i, j in itertools.combinations(range(n), 2):
      assert g[i] != g[j] or max(abs(y[i] - y[j]), abs(x[i] - x[j])) > r, case.name
    # every unchosen considered entry that outranks the last chosen one (every one, if the slots ran out) lies within the
    # radius of a chosen entry that outranks it (candidate 0 outranks everything: it is chosen first whatever its value)
    e = np.arange(N)
    eg, ey, ex = e // A, e % A // case.OH, e % case.OH
    ranked = cases.order(v[b, :N])
    rank = np.empty(N, np.int64)
    rank[ranked] = np.arange(N)
    rank_of = [-1] + [int(rank[c]) for c in chosen[1:]]
    last = rank_of[-1] if n == case.k and n > 1 else (N if n < case.k else -1)
    covered_by = np.full(N, N + 1)                                   # the best rank of a chosen entry that covers e
    for c in range(n):
      near = (eg == g[c]) & (np.abs(ey - y[c]) <= r) & (np.abs(ex - x[c]) <= r)
      covered_by[near] = np.minimum(covered_by[near], rank_of[c])
    must = (rank < last)
    must[[c for c in chosen if c < N]] = False
    assert np.all(covered_by[must] < rank[must]), case.name


def test_properties_of_the_restatement_and_select_reference_on_every_case():
  from stackrl_amd import candidates
  todo = cases.cases()
  assert len(todo) > 100
  for case in todo:
    v, a = cases.inputs(case)
    cand, count = cases.reference(v, a, case.k, case.radius, case.n_valid, case.OH)
    assert cand.dtype == np.int64 and count.dtype == np.int32
    if case.OH <= 33:
      _check_properties(case, v, a, cand, count)
    if case.radius > case.OH:
      assert np.all(count <= case.n_valid + (a is not None)), case.name             # exhaustion: one per map, and the action
    got = candidates.select_reference(torch.as_tensor(v), None if a is None else torch.as_tensor(a), k=case.k, radius=case.radius,
                                      n_valid=case.n_valid, OH=case.OH)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32
    assert np.array_equal(got[0].numpy(), cand) and np.array_equal(got[1].numpy(), count), case.name


def test_closed_forms():
  from stackrl_amd import candidates
  for select in (cases.reference, lambda v, a, k, r, n, OH: tuple(
      t.numpy() for t in candidates.select(torch.as_tensor(v), None if a is None else torch.as_tensor(a), k=k, radius=r, n_valid=n, OH=OH))):
    flat = np.full((1, 25), 3.0, np.float32)
    cand, count = select(flat, np.array([0]), 8, 1, 1, 5)
    assert cand.tolist() == [[0, 2, 4, 10, 12, 14, 20, 22]] and count.tolist() == [8]
    cand, count = select(flat, np.array([12]), 32, 2, 1, 5)
    assert cand.tolist() == [[12] * 32] and count.tolist() == [1]
    # a one-hot map without an action: the hot entry, then the constant rest in index order outside its neighbourhood
    hot = np.zeros((1, 25), np.float64)
    hot[0, 12] = 1.0
    cand, count = select(hot, None, 6, 1, 1, 5)
    assert cand.tolist() == [[12, 0, 2, 4, 10, 14]] and count.tolist() == [6]
    # the same with the action elsewhere: the hot entry comes second unless the action strikes it
    assert select(hot, np.array([24]), 3, 1, 1, 5)[0].tolist() == [[24, 12, 0]]
    assert select(hot, np.array([18]), 3, 1, 1, 5)[0].tolist() == [[18, 0, 2]]
    # other maps do not suppress: two constant 2 x 2 maps at a radius that covers a map
    two = np.ones((1, 8), np.float32)
    cand, count = select(two, None, 4, 5, 2, 2)
    assert cand.tolist() == [[0, 4, 0, 0]] and count.tolist() == [2]
    # an action in a map that is not considered strikes nothing considered; out of range, it is clamped
    assert select(two, np.array([5]), 3, 5, 1, 2)[0].tolist() == [[5, 0, 5]]
    assert select(two, np.array([99]), 2, 0, 2, 2)[0].tolist() == [[7, 0]]
    assert select(two, np.array([-3]), 2, 0, 2, 2)[0].tolist() == [[0, 1]]


def test_select_checks_its_arguments_and_converts_other_dtypes():
  from stackrl_amd import candidates
  v = torch.rand(2, 18)
  candidates.select(v, k=2, OH=3)
  for bad in (dict(k=0), dict(k=33), dict(radius=-1), dict(n_valid=3), dict(n_valid=0), dict(OH=4), dict(n_valid=1, OH=None),
              dict(action=torch.zeros(3, dtype=torch.int64))):
    with pytest.raises(ValueError):
      candidates.select(v, **dict(dict(k=2, OH=3), **bad))
  half = torch.rand(2, 3, 3, 2).to(torch.float16).permute(0, 3, 1, 2)              # not contiguous, not float32
  want = cases.reference(half.float().reshape(2, 18).numpy(), None, 4, 1, 2, 3)
  got = candidates.select(half, k=4, radius=1, n_valid=2, OH=3)
  assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])


# ---- the policy ----------------------------------------------------------------------------------------------------------

class _Base(object):
  def __init__(self, action, values):
    self.action, self.values, self.n_valid = torch.as_tensor(action), torch.as_tensor(values, dtype=torch.float32), []

  def __call__(self, obs, n_valid=None):
    self.n_valid.append(n_valid)
    return self.action, self.values


class _Evaluator(object):
  """Stands in for `Lookahead`: the reward of an action is looked up in a table [B, N]."""

  def __init__(self, k, table):
    self.k, self.table, self.calls = k, torch.as_tensor(table, dtype=torch.float32), []

  def evaluate(self, actions):
    self.calls.append(actions.clone())
    return self.table.gather(1, actions), torch.zeros_like(actions, dtype=torch.bool)


def _setting(G=2, OH=9, B=3, k=6, seed=3):
  v = cases.make_values('smooth', B, G, OH, 'float32', seed)
  a = np.array([int(np.nanargmax(v[b])) for b in range(B)])
  table = np.random.RandomState(seed).rand(B, G * OH * OH).astype(np.float32)
  obs = (torch.zeros(B, OH + 3, OH + 3, 2), torch.zeros(B, G, 4, 4, 1))      # H = OH + 3, h = 4: OH = H - h + 1
  return v, a, table, obs


def test_radius_none_calls_what_it_calls_today(monkeypatch):
  from stackrl_amd import candidates
  v, a, table, obs = _setting()
  monkeypatch.setattr(candidates, 'select', lambda *args, **kw: pytest.fail('radius=None must not reach candidates.select'))
  for n_valid in (None, 1):
    base, ev = _Base(a, v), _Evaluator(6, table)
    policy = la.LookaheadPolicy(base, ev, radius=None)
    action, values = policy(obs, n_valid=n_valid)
    want = la.candidates(torch.as_tensor(a), torch.as_tensor(v), 6, n_valid, 81 if n_valid else None)
    assert len(ev.calls) == 1 and torch.equal(ev.calls[0], want) and base.n_valid == [n_valid]
    assert torch.equal(action, la.choose(want, torch.as_tensor(table).gather(1, want))) and torch.equal(values, base.values)
    assert torch.equal(policy.last[0], want) and policy.last_count is None and policy.radius is None
    plain = la.LookaheadPolicy(_Base(a, v), _Evaluator(6, table))
    assert torch.equal(plain(obs, n_valid=n_valid)[0], action)


def test_radius_0_returns_the_actions_of_radius_none():
  v, a, table, obs = _setting()
  for n_valid in (None, 1, 2):
    ev0, ev = _Evaluator(6, table), _Evaluator(6, table)
    a0, _ = la.LookaheadPolicy(_Base(a, v), ev0, radius=0)(obs, n_valid=n_valid)
    a1, _ = la.LookaheadPolicy(_Base(a, v), ev)(obs, n_valid=n_valid)
    assert torch.equal(a0, a1) and torch.equal(ev0.calls[0], ev.calls[0])


def test_radius_3_evaluates_the_restatements_candidates_and_sets_last_count():
  v, a, table, obs = _setting()
  for n_valid, radius in ((None, 3), (1, 3), (2, 9)):
    base, ev = _Base(a, v), _Evaluator(6, table)
    policy = la.LookaheadPolicy(base, ev, radius=radius)
    action, values = policy(obs, n_valid=n_valid)
    cand, count = cases.reference(v, a, 6, radius, n_valid or 2, 9)
    assert len(ev.calls) == 1 and np.array_equal(ev.calls[0].numpy(), cand) and base.n_valid == [n_valid]
    assert policy.last_count.dtype == torch.int32 and np.array_equal(policy.last_count.numpy(), count)
    assert np.array_equal(policy.last[0].numpy(), cand) and torch.equal(values, base.values)
    want = la.choose(torch.as_tensor(cand), torch.as_tensor(table).gather(1, torch.as_tensor(cand)))
    assert torch.equal(action, want)
    if radius == 9:
      assert count.max() < 6                                # exhaustion: the repeats of candidate 0 never win a tie
    assert not np.array_equal(cand, la.candidates(torch.as_tensor(a), torch.as_tensor(v), 6, n_valid, 81 if n_valid else None).numpy())


def test_a_radius_needs_k_of_at_most_32():
  v, a, table, obs = _setting()
  with pytest.raises(ValueError, match='k <= 32'):
    la.LookaheadPolicy(_Base(a, v), _Evaluator(33, table), radius=2)
  with pytest.raises(ValueError):
    la.LookaheadPolicy(_Base(a, v), _Evaluator(4, table), radius=-1)
  la.LookaheadPolicy(_Base(a, v), _Evaluator(33, table))                 # without a radius k is not limited
