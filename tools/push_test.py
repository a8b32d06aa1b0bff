#!/usr/bin/env python3
"""Does the pile stand?  Run one batch of Stack-v0 episodes with a policy and, after every step, push a fork of every pile
(`stackrl_amd.push.PushTest`: the env itself is not touched) and note how many rocks moved.

  python tools/push_test.py [--policy height [random ...]] [--lookahead K] [--penalty X] [--speed 0.1] [--mode bump|shake|last]
                            [--substeps 50] [--trials 4] [--envs 128] [--episode-length 8] [--seed 11] [--out push]

--policy names methods of stackrl_amd.baselines; each is run on its own.  With --lookahead K > 1 the policy is the
`LookaheadPolicy` over the baseline's K best actions, and with --penalty X > 0 that lookahead pushes every candidate's pile
too and scores it `reward - X * moved / nb`.

Written under --out: `push.csv`, one line per policy, step, env and trial (step, env, trial, moved, max_perr, max_oerr,
at_rest; nb beside them), and `policies.csv`, per policy the mean return beside the mean moved / nb over its steps."""
import argparse
import csv
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PUSH_COLUMNS = ['policy', 'step', 'env', 'trial', 'nb', 'moved', 'max_perr', 'max_oerr', 'at_rest']


def make_policy(g, name, look_k, spec, penalty, seed):
  """(policy, what to close afterwards): the baseline `name`, behind a `LookaheadPolicy` of `look_k` candidates if look_k > 1,
  which pushes every candidate's pile and charges `penalty` per moved share if penalty > 0."""
  from stackrl_amd import baselines
  from stackrl_amd.lookahead import Lookahead, LookaheadPolicy
  rnd = seed if name == 'random' else None
  if look_k <= 1:
    return baselines.Baseline(name, seed=rnd), None
  look = Lookahead(g, look_k)
  pushing = penalty > 0
  return LookaheadPolicy(baselines.Baseline(name, value=True, seed=rnd), look, push=spec if pushing else None, penalty=penalty), look


def label(name, look_k, penalty):
  return name + ('+look{}'.format(look_k) if look_k > 1 else '') + ('+push{:g}'.format(penalty) if look_k > 1 and penalty > 0 else '')


def run_episode(g, policy, tester, spec, rows=None, tag=''):
  """One episode of every env: (mean return, mean moved / nb over the steps, envs and trials).  `rows`: a list that takes one
  PUSH_COLUMNS row per step, env and trial."""
  obs, _, _ = g.reset()
  ret = torch.zeros(g.batch_size, device=obs[0].device)
  shares = []
  for step in range(g.config.episode_length):
    a = policy(obs)
    obs, reward, done = g.step(a[0] if isinstance(a, tuple) else a)
    ret += reward
    d = tester.evaluate(spec)
    shares.append(d.moved_fraction.mean())
    if rows is not None:
      d = d.cpu()
      for e in range(d.moved.shape[0]):
        for t in range(d.moved.shape[1]):
          rows.append([tag, step, e, t, int(d.nb[e, t]), int(d.moved[e, t]), '{:.6g}'.format(float(d.max_perr[e, t])),
                       '{:.6g}'.format(float(d.max_oerr[e, t])), int(d.at_rest[e, t])])
  assert bool(done.all())
  return float(ret.mean()), float(torch.stack(shares).mean())


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--policy', nargs='+', default=['height'], help='methods of stackrl_amd.baselines (random, height, ...)')
  ap.add_argument('--lookahead', type=int, default=0, help='K > 1: choose among the K best actions by a simulated step')
  ap.add_argument('--penalty', type=float, default=0.0, help='X > 0: the lookahead pushes each candidate and charges X x moved / nb')
  ap.add_argument('--speed', type=float, default=0.1, help='m/s of the velocity increment')
  ap.add_argument('--mode', default='bump', choices=('bump', 'shake', 'last'))
  ap.add_argument('--substeps', type=int, default=50)
  ap.add_argument('--trials', type=int, default=4)
  ap.add_argument('--envs', type=int, default=128)
  ap.add_argument('--episode-length', type=int, default=8)
  ap.add_argument('--seed', type=int, default=11)
  ap.add_argument('--out', default='push')
  args = ap.parse_args()
  from stackrl_amd import env as envs
  from stackrl_amd.push import PushSpec, PushTest
  spec = PushSpec(speed=args.speed, substeps=args.substeps, mode=args.mode, seed=args.seed)
  os.makedirs(args.out, exist_ok=True)
  rows, table = [], []
  for name in args.policy:
    g = envs.VecStackEnv(n_parallel=args.envs, seed=args.seed, block=True, episode_length=args.episode_length)
    tester = PushTest(g, trials=args.trials)
    policy, look = make_policy(g, name, args.lookahead, spec, args.penalty, args.seed)
    tag = label(name, args.lookahead, args.penalty)
    ret, share = run_episode(g, policy, tester, spec, rows, tag)
    table.append([tag, '{:.6g}'.format(ret), '{:.6g}'.format(share)])
    print('{:28s} mean return {:8.4f}   mean moved / nb {:6.4f}  ({} envs x {} rocks, {} trials of {} at {} m/s, {} sub-steps)'.format(
      tag, ret, share, args.envs, args.episode_length, args.trials, args.mode, args.speed, args.substeps))
    for x in (look, tester, g):
      if x is not None:
        x.close()
  with open(os.path.join(args.out, 'push.csv'), 'w', newline='') as f:
    w = csv.writer(f)
    w.writerow(PUSH_COLUMNS)
    w.writerows(rows)
  with open(os.path.join(args.out, 'policies.csv'), 'w', newline='') as f:
    w = csv.writer(f)
    w.writerow(['policy', 'mean_return', 'mean_moved_share'])
    w.writerows(table)
  print('wrote {} and {}'.format(os.path.join(args.out, 'push.csv'), os.path.join(args.out, 'policies.csv')))


if __name__ == '__main__':
  main()
