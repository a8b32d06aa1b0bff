"""CPU tests of the lookahead policy's rules and of `EnvState` as a value: `LookaheadPolicy` on CPU tensors with a stand-in
evaluator (no env, no device), the `state_dict` round trip, and the host checks of `set_state` (`state.plan_set`)."""
import io

import pytest

torch = pytest.importorskip('torch')

from stackrl_amd import lookahead as la  # noqa: E402
from stackrl_amd import state as st  # noqa: E402


class _Base(object):
  """A base policy that returns what it was given."""

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


_OBS = (torch.zeros(2, 4, 4, 2), torch.zeros(2, 3, 2, 2, 1))      # two envs, three object maps (grouped)


def test_candidates_are_ordered_by_value_with_ties_to_the_lower_index():
  values = [[1., 5., 5., 0., 5., 2.], [3., 3., 3., 3., 3., 3.]]
  c = la.candidates(torch.tensor([1, 0]), torch.tensor(values), 4)
  assert c.tolist() == [[1, 2, 4, 5], [0, 1, 2, 3]]
  # k as large as the map: every entry once, the base's first
  c = la.candidates(torch.tensor([3, 5]), torch.tensor(values), 6)
  assert c.tolist() == [[3, 1, 2, 4, 5, 0], [5, 0, 1, 2, 3, 4]]
  with pytest.raises(ValueError):
    la.candidates(torch.tensor([0, 0]), torch.tensor(values), 7)


def test_candidate_0_is_the_base_action_even_when_it_is_not_the_arg_max():
  values = [[1., 9., 8., 7., 0., 2.], [0., 1., 2., 3., 4., 5.]]
  c = la.candidates(torch.tensor([4, 2]), torch.tensor(values), 3)
  assert c.tolist() == [[4, 1, 2], [2, 5, 4]]           # the base's own action, then the map's best others
  c = la.candidates(torch.tensor([2, 5]), torch.tensor(values), 3)
  assert c.tolist() == [[2, 1, 3], [5, 4, 3]]           # inside the top k: it moves to the front, nothing comes twice
  assert la.candidates(torch.tensor([[4], [2]]), torch.tensor(values).reshape(2, 2, 3), 2).tolist() == [[4, 1], [2, 5]]


def test_n_valid_masks_the_maps_that_are_not_on_show():
  # three maps of two entries; the best values sit in the last map, which is not on show
  values = [[1., 2., 3., 4., 9., 9.], [4., 3., 2., 1., 9., 9.]]
  c = la.candidates(torch.tensor([0, 3]), torch.tensor(values), 3, n_valid=2, n_actions=2)
  assert c.tolist() == [[0, 3, 2], [3, 0, 1]]
  base = _Base([0, 3], values)
  ev = _Evaluator(3, [[0.] * 6] * 2)
  policy = la.LookaheadPolicy(base, ev)
  a, v = policy(_OBS, n_valid=2)
  assert base.n_valid == [2] and ev.calls[0].tolist() == [[0, 3, 2], [3, 0, 1]] and int(ev.calls[0].max()) < 4
  assert a.tolist() == [0, 3] and v is not None
  with pytest.raises(ValueError):
    la.candidates(torch.tensor([0, 3]), torch.tensor(values), 5, n_valid=2, n_actions=2)       # only four entries on show


def test_the_highest_simulated_reward_wins_with_ties_to_the_lower_rank():
  values = [[0., 1., 2., 3., 4., 5.], [5., 4., 3., 2., 1., 0.]]
  base = _Base([0, 0], values)
  #                                 candidates: [0, 5, 4, 3]               [0, 1, 2, 3]
  ev = _Evaluator(4, [[.1, 0., 0., .7, .7, .2], [.3, .3, .1, .3, 0., 0.]])
  a, v = la.LookaheadPolicy(base, ev)(_OBS)
  assert ev.calls[0].tolist() == [[0, 5, 4, 3], [0, 1, 2, 3]]
  assert a.tolist() == [4, 0]                # .7 twice: rank 2 (action 4) before rank 3; .3 three times: the base's own
  assert torch.equal(v, base.values) and base.n_valid == [None]
  assert la.choose(torch.tensor([[7, 8, 9]]), torch.tensor([[float('-inf')] * 3])).tolist() == [7]


def test_k_1_is_the_base_policy():
  values = torch.rand(2, 6)
  base = _Base([4, 1], values)
  ev = _Evaluator(1, torch.zeros(2, 6))
  a, v = la.LookaheadPolicy(base, ev)(_OBS)
  assert a.tolist() == [4, 1] and torch.equal(v, values) and ev.calls == []      # nothing is simulated


def _state(n=3, words=8, left=5, signature=0xfeedfacecafebeef, extra=None):
  g = torch.Generator().manual_seed(n)
  return st.EnvState(torch.randint(-2 ** 31, 2 ** 31 - 1, (n, words), dtype=torch.int32, generator=g),
                     (torch.randint(0, 255, (n, 4, 4, 2), dtype=torch.uint8, generator=g), torch.randint(0, 255, (n, 2, 2, 1), dtype=torch.uint8, generator=g)),
                     torch.rand(n, generator=g), torch.tensor([False, True, False][:n]), left, 4294967295, 7, signature, extra)


def test_state_dict_survives_torch_save_and_load():
  s = _state(extra={'since_reset': 2, 'done_prev': torch.tensor([True, False, False]), 'len_rng_keys': torch.arange(624), 'len_rng_pos': 9,
                    'len_rng_has_gauss': 0, 'len_rng_gauss': 0.0})
  d = s.state_dict()
  assert all(torch.is_tensor(v) or isinstance(v, (int, float)) for v in d.values())      # plain tensors and numbers
  buf = io.BytesIO()
  torch.save(d, buf)
  buf.seek(0)
  t = st.EnvState.from_state_dict(torch.load(buf, weights_only=True))
  assert (t.left, t.seed, t.sample_counter, t.signature) == (5, 4294967295, 7, 0xfeedfacecafebeef) and len(t) == 3
  for a, b in ((s.records, t.records), (s.obs[0], t.obs[0]), (s.obs[1], t.obs[1]), (s.reward, t.reward), (s.done, t.done),
               (s.extra['done_prev'], t.extra['done_prev']), (s.extra['len_rng_keys'], t.extra['len_rng_keys'])):
    assert a.dtype == b.dtype and torch.equal(a, b)
  assert {k: v for k, v in t.extra.items() if not torch.is_tensor(v)} == {k: v for k, v in s.extra.items() if not torch.is_tensor(v)}
  u = t.cpu().to('cpu')
  assert torch.equal(u.records, s.records) and u.extra['since_reset'] == 2
  (om, oo), r, d = s.step_tuple([2, 2, 0])
  assert torch.equal(om, s.obs[0][[2, 2, 0]]) and torch.equal(r, s.reward[[2, 2, 0]]) and d.tolist() == [False, False, False]


def test_set_state_checks():
  s = _state()
  sig = s.signature
  assert st.plan_set(s, sig, 5, 3) == (None, None, True)                         # the whole batch, in order
  assert st.plan_set(s, sig, 0, 6, source=[0, 0, 1, 1, 2, 2]) == (None, [0, 0, 1, 1, 2, 2], True)      # forked over a batch; its own `left`
  assert st.plan_set(s, sig, 5, 8, indexes=torch.tensor([7, 0]), source=[1, 1]) == ([7, 0], [1, 1], False)
  assert st.plan_set(s, sig, 5, 8, indexes=[1, 4, 2]) == ([1, 4, 2], None, False)
  with pytest.raises(ValueError, match='point of the episode'):
    st.plan_set(s, sig, 4, 8, indexes=[1, 4, 2])                                 # a partial set at another episode point
  with pytest.raises(ValueError, match='distinct'):
    st.plan_set(s, sig, 5, 8, indexes=[1, 4, 1])                                 # repeated destinations
  with pytest.raises(ValueError, match='signature'):
    st.plan_set(s, sig ^ 1, 5, 3)                                                # a foreign signature
  with pytest.raises(ValueError, match='signature'):
    st.plan_set(s, sig ^ (1 << 63), 5, 8, indexes=[0, 1, 2])
  with pytest.raises(ValueError):
    st.plan_set(s, sig, 5, 4)                                                    # three records for four envs
  with pytest.raises(ValueError):
    st.plan_set(s, sig, 5, 8, indexes=[0, 8, 1])                                 # an env outside the batch
  with pytest.raises(ValueError):
    st.plan_set(s, sig, 5, 8, indexes=[0, 1], source=[0, 3])                     # a record outside the state
  with pytest.raises(ValueError):
    st.plan_set(s, sig, 5, 8, indexes=[0, 1])                                    # two envs for three records
