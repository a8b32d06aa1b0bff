"""GPU tests of libstackrl_valueview.so: every byte of the frames equals tests/value_view_cases.py's restatement of
include/stackrl_valueview.h — on synthetic tensors over the shapes at which the kernels take another path, on the committed
matplotlib maps, and through `compare.run(..., visualize=...)` on real envs."""
import numpy as np
import pytest
import torch

import value_view_cases as cases

pytestmark = pytest.mark.gpu

CASES = cases.device_cases()
SENTINEL = 0x5a


def _device_frames(p, inputs, sentinel=SENTINEL):
  from stackrl_amd import valueview
  rgb0, rgb1, values, actions = inputs
  dev = torch.device('cuda', 0)
  view = valueview.ValueView(scale=p['scale'], mark=p['mark'])
  B = rgb0.shape[0]
  n = B if p['indexes'] is None else len(p['indexes'])
  l = valueview.layout(p['H'], p['h'], len(values), p['scale'])
  out = torch.full((n, l['FH'], l['FW'], 3), sentinel, dtype=torch.uint8, device=dev)
  got = view.frames(torch.as_tensor(rgb0).to(dev), torch.as_tensor(rgb1).to(dev), [torch.as_tensor(v).to(dev) for v in values],
                    None if actions is None else [torch.as_tensor(a).to(dev) for a in actions], index=p['index'],
                    indexes=p['indexes'], out=out)
  assert got is out
  return out.cpu().numpy()


def test_the_cases_cover_what_the_kernels_turn_on():
  ps = [p for _, p in CASES]
  sizes = []
  for p in ps:
    l = cases.layout(p['H'], p['h'], p['P'], p['scale'])
    n = p['B'] if p['indexes'] is None else len(p['indexes'])
    sizes.append(n * l['FH'] * l['FW'] * 3)
  assert {s % 4 for s in sizes} == {0, 1, 2, 3}                      # whole words only, and every length of tail
  assert {(p['H'], p['h']) for p in ps} >= {(16, 8), (32, 8), (128, 32)}
  assert {p['scale'] for p in ps} >= {1, 2, 3} and {p['P'] for p in ps} >= {1, 3, 4, 6, 8}
  assert {p['index'] for p in ps if p['P'] == 8} == set(range(8))
  assert {p['G'] for p in ps} >= {1, 4} and any(p['indexes'] == [4, 0, 4] and p['B'] == 5 for p in ps)
  assert any(p['f64_mask'] not in (0, 2 ** p['P'] - 1) for p in ps) and {p['mark'] for p in ps} == {False, True}
  assert any(not p['with_actions'] for p in ps)
  p = next(p for p in ps if p['corners'])
  pixels = cases.case_inputs(p)[3] % 81
  assert set(pixels.ravel()) == {0, 8, 72, 80}                        # a pixel in each corner of the action map
  p = next(p for p in ps if p['G'] == 4 and p['B'] >= 3)
  rows = cases.case_inputs(p)[3] // ((p['H'] - p['h'] + 1) ** 2)
  assert len(set(rows[0])) > 1 and len(set(rows[:, 0])) > 1           # different rows per env and per policy


@pytest.mark.parametrize('tag,p', CASES, ids=[t for t, _ in CASES])
def test_frames_equal_the_restatement(tag, p):
  inputs = cases.case_inputs(p)
  want = cases.case_frames(p, inputs)
  got = _device_frames(p, inputs)
  assert got.shape == want.shape and got.dtype == np.uint8
  assert np.array_equal(got, want)
  # every byte is written: a second sentinel gives the same bytes
  assert np.array_equal(_device_frames(p, inputs, sentinel=0xa5), want)


def test_the_committed_maps_come_out_in_matplotlibs_bytes():
  inputs = cases.fixture_inputs()
  g = cases.golden()
  M = len(g['maps'])
  p = dict(H=16, h=8, P=2, scale=1, index=1, indexes=None, mark=False)
  got = _device_frames(p, inputs)
  assert np.array_equal(got, cases.case_frames(p, inputs))
  reg = cases.regions(16, 8, 2, 1)
  for k, order in ((0, range(M)), (1, range(M - 1, -1, -1))):          # policy 1 holds the maps reversed, in float64
    r0, r1, c0, c1 = reg['tile{}'.format(k)]
    for b, m in enumerate(order):
      cells = got[b, r0 + 3:r1 - 3, c0 + 3:c1 - 3]
      fin = np.isfinite(g['maps'][m])
      assert np.array_equal(cells[fin], g['rgba'][m][..., :3][fin]), g['names'][m]
      assert np.all(cells[~fin] == 255), g['names'][m]


def test_api_refusals_on_the_device():
  from stackrl_amd import valueview
  dev = torch.device('cuda', 0)
  rgb0, rgb1, values, actions = [torch.as_tensor(x).to(dev) if isinstance(x, np.ndarray) else x for x in cases.synthetic(2, 16, 8, 2, G=2)]
  values = [torch.as_tensor(v).to(dev) for v in values]
  view = valueview.ValueView()
  with pytest.raises(ValueError, match='need the actions'):
    view.frames(rgb0, rgb1, values)
  with pytest.raises(ValueError, match='uint8'):
    view.frames(rgb0.float(), rgb1, values, list(actions))
  with pytest.raises(RuntimeError, match='index must be in 0..1, got 2'):
    view.frames(rgb0, rgb1, values, list(actions), index=2)
  with pytest.raises(ValueError, match='scale must be in 1..8'):
    valueview.ValueView(scale=9)


def _run_case(ref_pool, tmp_path, **env_kwargs):
  from stackrl_amd import compare, env as envs, valueview
  from stackrl_amd.baselines import Baseline
  seen = []

  class Keep(object):
    envs = (3, 0)
    view = valueview.ValueView(scale=1, mark=True)

    def __call__(self, step, index, frames):
      seen.append((step, index, frames.cpu().numpy(), [t.cpu().numpy() for t in env.render('rgb_array', dtype='uint8')]))

  def make():
    return envs.make('Stack-v0' if 'orientation_freedom' not in env_kwargs else 'Stack-v2', n_parallel=4, resolution_factor=3,
                     episode_length=3, pool=ref_pool, block=True, **env_kwargs)

  def policies():
    return {'height': Baseline('height', value=True), 'random': Baseline('random', value=True, seed=3)}
  env = make()
  try:
    plain = compare.run(env, policies(), num_steps=3, keep_values=True)
  finally:
    env.close()
  env = make()
  try:
    shown = compare.run(env, policies(), num_steps=3, keep_values=True, visualize=Keep())
  finally:
    env.close()
  env = make()
  try:
    rec = valueview.Recorder(str(tmp_path), envs=(1,), scale=2)
    recorded = compare.run(env, policies(), num_steps=3, visualize=rec)
  finally:
    env.close()
  # the returned dict does not depend on `visualize`
  assert sorted(plain) == sorted(shown)
  for k in plain:
    assert plain[k].dtype == shown[k].dtype and np.array_equal(plain[k], shown[k], equal_nan=plain[k].dtype.kind == 'f') \
      if isinstance(plain[k], np.ndarray) else plain[k] == shown[k], k
  assert plain['record'].tobytes() == shown['record'].tobytes() == recorded['record'].tobytes()
  # the frames are the restatement applied to what the env rendered and the values the run kept
  assert [(s, i) for s, i, _, _ in seen] == [(s, i) for i in range(2) for s in range(3)]
  A = plain['n_actions']
  OH = int(round(A ** 0.5))
  for t, (step, index, frames, (rgb0, rgb1)) in enumerate(seen):
    values = [shown['values'][j, t].reshape(4, 1, A) for j in range(2)]
    pixels = shown['actions'][:, t].astype(np.int64)
    actions = pixels[..., 0] * OH + pixels[..., 1]                      # row 0 of the kept (chosen) maps
    want = cases.reference_frames(rgb0, rgb1, values, actions, index=index, indexes=[3, 0], scale=1, mark=True)
    assert np.array_equal(frames, want), (step, index)
  # the recorder's files
  stacked = np.load(str(tmp_path / 'frames.npy'))
  l = valueview.layout(rgb0.shape[1], rgb1.shape[1], 2, 2)
  assert stacked.shape == (2, 3, 1, l['FH'], l['FW'], 3) and stacked.dtype == np.uint8
  with open(str(tmp_path / 'policy1_step2_env1.ppm'), 'rb') as f:
    data = f.read()
  head = 'P6\n{} {}\n255\n'.format(l['FW'], l['FH']).encode()
  assert data.startswith(head) and data[len(head):] == stacked[1, 2, 0].tobytes()
  assert len(list(tmp_path.glob('*.ppm'))) == 6


def test_a_visualised_run_on_stack_v0(ref_pool, tmp_path):
  _run_case(ref_pool, tmp_path)


def test_a_visualised_run_on_the_grouped_observation(ref_pool, tmp_path):
  _run_case(ref_pool, tmp_path, orientation_freedom=1)
