#!/usr/bin/env python3
"""Compare the heuristic baselines, and optionally a Q-network with saved weights, on one env: the reference's `test` command
(`python -m stackrl test`; stackrl/test.py) through `stackrl_amd.compare`.  Prints the return table and the P x P matrices,
and writes `results.csv` (and `data.npz`) under `--save`.

  python tools/compare_policies.py [--env Stack-v0] [--envs 16] [--num-steps 64] [--episode-length 8]
                                   [--baselines random,height,difference,corrcoef] [--weights FILE] [--save DIR] [--plots]
                                   [--lookahead K [--spread R]] [--visualize DIR [--show 0,1] [--scale 2] [--mark]]

`--lookahead K` adds `<name>+look<K>` beside every policy: of the policy's own action and the K - 1 best other entries of its
value map, the one whose simulated step gives the highest reward (stackrl_amd/lookahead.py).  With `--spread R` the policies
are named `<name>+look<K>r<R>` and their candidates are spread: each strikes the entries of its map within R pixels, and the
next is the best entry left (stackrl_amd/candidates.py).

`--visualize DIR` writes the picture of the reference's `-v/--visualize` for the envs of `--show` at every step, drawn on the
device (stackrl_amd/valueview.py): `DIR/policy<p>_step<t>_env<i>.ppm` and `DIR/frames.npy`.  A frame holds the overhead view,
the object view below it and one tile per policy, the driving policy's framed; frames carry no text, so the order of the tiles is
printed.  `--mark` also draws each policy's chosen pixel, and the driving policy's window in the overhead view, in red.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stackrl_amd import compare  # noqa: E402
from stackrl_amd.baselines import Baseline  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--env', default='Stack-v0', choices=('Stack-v0', 'Stack-v1', 'Stack-v2'))
  ap.add_argument('--envs', type=int, default=16)
  ap.add_argument('--num-steps', type=int, default=64)
  ap.add_argument('--episode-length', type=int, default=8)
  ap.add_argument('--seed', type=int, default=11)
  ap.add_argument('--baselines', default='random,height,difference,corrcoef')
  ap.add_argument('--weights', default=None, help='a file written by DQN.save_weights: adds the greedy policy of that network')
  ap.add_argument('--save', default=os.path.join('data', 'test'))
  ap.add_argument('--plots', action='store_true')
  ap.add_argument('--keep-values', action='store_true')
  ap.add_argument('--lookahead', type=int, default=0, metavar='K', help='adds <name>+look<K> beside every policy')
  ap.add_argument('--spread', type=int, default=None, metavar='R', help='with --lookahead: spread the candidates by radius R; names <name>+look<K>r<R>')
  ap.add_argument('--visualize', default=None, metavar='DIR', help='write the frames of a visualised run under DIR')
  ap.add_argument('--show', default='0', help='with --visualize: comma-separated env indices whose frames are written')
  ap.add_argument('--scale', type=int, default=2, help='with --visualize: output pixels per source pixel (1..8)')
  ap.add_argument('--mark', action='store_true', help='with --visualize: mark the chosen pixels in red')
  args = ap.parse_args()
  if args.spread is not None and (args.lookahead < 1 or args.spread < 0):
    raise SystemExit('--spread needs --lookahead K and a radius of at least 0')
  if not torch.cuda.is_available():
    raise SystemExit('compare_policies needs a HIP device')
  policies = {m: Baseline(m, value=True, seed=3 if m == 'random' else None) for m in args.baselines.split(',') if m}
  env_kwargs = dict(env=args.env, n_parallel=args.envs, episode_length=args.episode_length, block=True)
  if args.weights:
    from stackrl_amd import env as envs, nets, qops
    from stackrl_amd.dqn import DQN
    probe = envs.make(**env_kwargs)
    spec = probe.observation_spec
    probe.close()
    if len(spec[1].shape) == 4:                        # Stack-v2: the network sees one object map
      spec = (spec[0], type(spec[1])(tuple(spec[1].shape[1:]), spec[1].dtype))
    net = nets.DeepQSiamFCN(spec, seed=0).cuda()
    net.load_state_dict(torch.load(args.weights, map_location='cuda'))
    agent = DQN(net, collect_batch_size=args.envs, replay_memory_size=2 * args.envs, seed=0, policy_op=qops.FusedPolicy(fast=True),
                xcorr='bf16x3')
    policies['dqn'] = lambda obs, n_valid=None: agent.greedy(obs, values=True, n_valid=n_valid)
  looks = []

  def with_lookahead(env, policies):
    from stackrl_amd.lookahead import Lookahead, LookaheadPolicy
    looks.append(Lookahead(env, args.lookahead))
    out = {}
    for name, p in policies.items():
      out[name] = p
      if args.spread is None:
        out['{}+look{}'.format(name, args.lookahead)] = LookaheadPolicy(p, looks[0])
      else:
        out['{}+look{}r{}'.format(name, args.lookahead, args.spread)] = LookaheadPolicy(p, looks[0], radius=args.spread)
    return out
  recorder = None
  if args.visualize:
    from stackrl_amd import valueview
    shown = [int(i) for i in args.show.split(',') if i != '']
    if not shown or min(shown) < 0 or max(shown) >= args.envs:
      raise SystemExit('--show must name envs in 0..{}'.format(args.envs - 1))
    recorder = valueview.Recorder(args.visualize, envs=shown, scale=args.scale, mark=args.mark)
  res = compare.test(policies, num_steps=args.num_steps, seed=args.seed, save=args.save, plots=args.plots,
                     keep_values=args.keep_values, with_env=with_lookahead if args.lookahead > 0 else None,
                     visualize=recorder, **env_kwargs)
  if recorder:
    names = [str(k) for k in res['keys']]
    print('frames: {} files under {} ({} x {} pixels); tiles, left to right and line by line, when a policy drives:'.format(
      len(recorder.frames) * len(recorder.envs) + 1, args.visualize, *recorder.frames[0][2].shape[1:3][::-1]))
    for i, name in enumerate(names):
      print('  policy{} {}: {}'.format(i, name, ', '.join('[{}]'.format(n) if n == name else n for n in valueview.tile_order(names, i))))
  for look in looks:
    look.close()
  np.set_printoptions(precision=3, suppress=True, linewidth=160)
  print('{:>12} {:>10} {:>10} {:>12} {:>12}'.format('policy', 'return', '+/-', 'action value', '+/-'))
  for row in zip(res['keys'], res['return'], res['return_std'], res['action_value'], res['action_value_std']):
    print('{:>12} {:>10.4f} {:>10.4f} {:>12.4f} {:>12.4f}'.format(*row))
  for k in ('distance', 'corrcoef', 'overlap_mean', 'overlap_std'):
    print(k)
    print(res[k])
  path = os.path.join(args.save, compare_path(env_kwargs), 'results.csv')
  print('results:', path)
  print(open(path).read())


def compare_path(env_kwargs):
  from stackrl_amd import env as envs
  return envs.env_path(**{k: v for k, v in env_kwargs.items() if k not in ('n_parallel', 'block', 'pool', 'device')})


if __name__ == '__main__':
  main()
