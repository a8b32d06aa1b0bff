#!/usr/bin/env python3
"""Golden images of `StackEnv.render('rgb_array')` (env.py:295-332) and `TestStackEnv.render` (env.py:558-596) from the
reference's OWN code, run over the scripted pybullet stand-in of `make_rewarder_golden.py` (which see: the reference's
observer.py, rewarder.py and env.py are loaded by file path and run as they are; what pybullet would compute is scripted).

Runs only in the build container (needs /root/reference).  `TestStackEnv` also reads `Box.high` and iterates and indexes its
`Tuple` spaces (env.py:465-470, :598-608), so the two placeholders get those here.

The file written (`view_golden.npz`) holds data only, at a tiny resolution (`resolution_factor=2`: 16 x 16 and 4 x 4 maps):
per case the inputs — `Observer.state` (overhead map, object map or the list of them) and the goal rectangle — and the two
images the reference returned.  The cases cover an empty scene (overhead max 0: the `_max != 0` branch), scenes with rocks, no
rock pending, and goals that touch the map's edges.  tests/test_view.py holds tests/view_cases.py to them bit for bit."""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_rewarder_golden as mrg      # noqa: E402

OUT = os.path.join(HERE, 'view_golden.npz')


class Box(object):
  def __init__(self, low=0, high=1, dtype=None, shape=None):
    self.shape, self.dtype = shape, dtype
    self.low, self.high = np.full(shape, low), np.full(shape, high)


class Tuple(object):
  def __init__(self, spaces):
    self.spaces = tuple(spaces)

  def __getitem__(self, i):
    return self.spaces[i]

  def __iter__(self):
    return iter(self.spaces)

  def contains(self, x):
    return len(x) == len(self.spaces) and all(s.contains(int(a)) for s, a in zip(self.spaces, x))


def record(out, tag, env, test_env):
  m, n = env._obs.state
  (u0, v0), (u1, v1) = env._rew._goal_lims
  rgb0, rgb1 = env.render('rgb_array')
  assert rgb0.dtype == np.float64 and rgb1.dtype == np.float64 and np.asarray(m).dtype == np.float32
  assert np.array_equal(np.argwhere(env._rew.goal_bin), np.argwhere(np.pad(np.ones((u1 - u0, v1 - v0), bool), ((u0, m.shape[0] - u1), (v0, m.shape[1] - v1)))))
  out[tag + '_m'] = np.asarray(m)
  out[tag + '_n'] = np.stack(n) if test_env else np.asarray(n)      # `TestStackEnv.render` colours n[0]
  out[tag + '_goal'] = np.array((u0, v0, u1 - u0, v1 - v0), np.int32)
  out[tag + '_rgb0'], out[tag + '_rgb1'] = rgb0, rgb1
  return tag


def main():
  rng = np.random.RandomState(23)
  draws = mrg.ScriptedDraws(mrg.goal_draws(rng))
  ref = mrg.load_reference(draws)
  ref['env'].spaces.Box, ref['env'].spaces.Tuple = Box, Tuple
  mrg.StubSimulator.script_rng = rng
  h = 4                                                           # resolution_factor=2
  mrg.StubSimulator.res = (4 * h, h)
  full = dict(dtype='uint8', goal_size_ratio=.25, reward_params=2, seed=5, episode_length=3, resolution_factor=2)
  out, tags = {}, []
  AW = 3 * h + 1

  def aim(env):                                                   # a pixel inside the goal, so that rocks pile up in view
    (gu0, gv0), (gu1, gv1) = env._rew._goal_lims
    return int(np.clip(rng.randint(gu0, gu1) - h // 2, 0, AW - 1)) * AW + int(np.clip(rng.randint(gv0, gv1) - h // 2, 0, AW - 1))

  # StackEnv: four episodes (the four fixed goal draws: the ends of every range), rendered after the reset, after every
  # placement and after the last one, when no rock is pending
  env = ref['env'].StackEnv(**full)
  for ep in range(4):
    env.reset()
    tags.append(record(out, 'v0_e{}_reset'.format(ep), env, False))
    for k in range(full['episode_length'] + 1):
      _, _, done, _ = env.step(aim(env))
      tags.append(record(out, 'v0_e{}_s{}'.format(ep, k), env, False))
      if done:
        break
    assert done
  env.close()
  # TestStackEnv with two orientations
  env = ref['env'].TestStackEnv(orientation_freedom=1, **full)
  for ep in range(2):
    env.reset()
    tags.append(record(out, 'v2_e{}_reset'.format(ep), env, True))
    for k in range(full['episode_length'] + 1):
      if env._obs.num_objects == 0:
        break
      _, _, done, _ = env.step((int(rng.randint(env._obs.num_objects)), aim(env)))
      tags.append(record(out, 'v2_e{}_s{}'.format(ep, k), env, True))
      if done:
        break
  env.close()
  out['cases'] = np.array(tags)
  for t in tags:
    print(' ', t, 'goal', out[t + '_goal'], 'max m %.4f' % out[t + '_m'].max(), 'n', out[t + '_n'].shape, 'max n %.6g' % out[t + '_n'].max())
  # what the cases must cover
  H = 4 * h
  assert any(out[t + '_m'].max() == 0 for t in tags) and any(out[t + '_m'].max() > 0 for t in tags)
  g = np.array([out[t + '_goal'] for t in tags])
  # (the first row, the first column and the last column; the draws never make a goal as tall as this map)
  assert (g[:, 0] == 0).any() and (g[:, 1] == 0).any() and (g[:, 1] + g[:, 3] == H).any()
  assert any(out[t + '_n'].max() == 0 for t in tags)
  assert (g[:, 2] != g[:, 3]).any()
  np.savez_compressed(OUT, **out)
  print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(tags), 'cases')


if __name__ == '__main__':
  main()
