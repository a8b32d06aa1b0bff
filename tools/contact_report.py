#!/usr/bin/env python3
"""Who rests on whom: run N Stack-v0 envs for one episode — with a heuristic baseline, with the greedy policy of a Q-network's
saved weights, or on one pixel (--pixel centre) — and after every placement print the contact table of one env
(`env.contact_points(wrench=True)`: pybullet's getContactPoints for the whole pile) and write it as CSV.

  python tools/contact_report.py [--envs 4] [--episode-length 8] [--baseline height | --weights FILE | --pixel centre]
                                 [--show 0] [--out contacts] [--seed 11]

Written under --out: `contacts.csv`, one line per step and contact (step, a, b, positions, normal, distance, forces and
directions), and `bodies.csv`, one line per step and body:
  supports      the bodies below it that it rests on (-1 = the ground): the other body of its contacts whose force on it points up
  carries       the bodies resting on it
  points        its contact points
  normal_load   the sum of the normal forces of all its contacts, N
  support_up    the upward contact force on it from its supports, N
  weight        its mass x gravity, N
  share         support_up / weight: 1 for a body at rest that carries nothing, more for one that carries others"""
import argparse
import csv
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONTACT_COLUMNS = ['step', 'a', 'b', 'ax', 'ay', 'az', 'bx', 'by', 'bz', 'nx', 'ny', 'nz', 'distance', 'normal_force',
                   'friction1', 't1x', 't1y', 't1z', 'friction2', 't2x', 't2y', 't2z']
BODY_COLUMNS = ['step', 'body', 'mesh', 'supports', 'carries', 'points', 'normal_load', 'support_up', 'weight', 'share']


def body_table(bodies, rows, nb, mesh_ids, masses, gravity):
  """Per body slot a dict of BODY_COLUMNS (without the step) from one env's contacts: bodies int [n, 2], rows float [n, 20]."""
  out = []
  n = rows[:, 6:9]
  F = n * rows[:, 10:11] + rows[:, 12:15] * rows[:, 11:12] + rows[:, 16:19] * rows[:, 15:16]      # on A; -F on B
  for b in range(nb):
    supports, carries, load, up = set(), set(), 0.0, 0.0
    points = 0
    for k in range(len(rows)):
      if bodies[k, 0] == b:
        other, fz = int(bodies[k, 1]), float(F[k, 2])
      elif bodies[k, 1] == b:
        other, fz = int(bodies[k, 0]), -float(F[k, 2])
      else:
        continue
      points += 1
      load += float(rows[k, 10])
      if fz > 0:
        supports.add(other)
        up += fz
      elif fz < 0:
        carries.add(other)
    weight = float(masses[mesh_ids[b]]) * gravity
    out.append(dict(body=b, mesh=int(mesh_ids[b]), supports=' '.join(str(s) for s in sorted(supports)),
                    carries=' '.join(str(s) for s in sorted(carries)), points=points, normal_load=load, support_up=up, weight=weight,
                    share=up / weight if weight > 0 else float('nan')))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4)
  ap.add_argument('--episode-length', type=int, default=8)
  ap.add_argument('--seed', type=int, default=11)
  ap.add_argument('--baseline', default='height', help='a method of stackrl_amd.baselines (random, height, difference, corrcoef, ...)')
  ap.add_argument('--weights', default=None, help='saved Q-network weights: the greedy policy instead of a baseline')
  ap.add_argument('--pixel', default=None, help="'centre' or a flat action index: every rock on that pixel instead of a policy")
  ap.add_argument('--show', type=int, default=0, help='the env whose table is printed and written')
  ap.add_argument('--out', default='contacts')
  args = ap.parse_args()
  from stackrl_amd import baselines, env as envs
  g = envs.VecStackEnv(n_parallel=args.envs, seed=args.seed, block=True, episode_length=args.episode_length)
  if not 0 <= args.show < args.envs:
    raise SystemExit('--show must name one of the {} envs'.format(args.envs))
  if args.pixel is not None:
    aw = g.config.overhead_res - g.config.object_res + 1
    a = (aw // 2) * aw + aw // 2 if args.pixel == 'centre' else int(args.pixel)
    policy = lambda obs: torch.full((args.envs,), a, dtype=torch.int64, device='cuda')
  elif args.weights:
    from stackrl_amd import nets, qops
    from stackrl_amd.dqn import DQN
    net = nets.DeepQSiamFCN(g.observation_spec, seed=0).cuda()
    net.load_state_dict(torch.load(args.weights, map_location='cuda'))
    policy = DQN(net, collect_batch_size=args.envs, replay_memory_size=2 * args.envs, seed=0, policy_op=qops.FusedPolicy(fast=True),
                 xcorr='bf16x3').greedy
  else:
    policy = baselines.Baseline(args.baseline, seed=args.seed if args.baseline == 'random' else None)
  os.makedirs(args.out, exist_ok=True)
  masses, gravity = g.pool.mass_com[:, 0], float(g.config.gravity)
  obs, _, _ = g.reset()
  with open(os.path.join(args.out, 'contacts.csv'), 'w', newline='') as fc, open(os.path.join(args.out, 'bodies.csv'), 'w', newline='') as fb:
    wc, wb = csv.writer(fc), csv.DictWriter(fb, ['step'] + BODY_COLUMNS[1:])
    wc.writerow(CONTACT_COLUMNS)
    wb.writeheader()
    for step in range(args.episode_length):
      obs, reward, done = g.step(policy(obs))
      cp = g.contact_points(wrench=True).cpu()
      e = args.show
      n = int(cp.count[e])
      bodies, rows = cp.bodies[e, :n].numpy(), cp.rows[e, :n].numpy().astype(np.float64)
      poses, nb, _, _ = g.state()
      print('step {}: env {} holds {} bodies and {} contacts ({} with the ground)'.format(step, e, int(nb[e]), n, int((bodies[:, 1] < 0).sum())))
      for k in range(n):
        wc.writerow([step, bodies[k, 0], bodies[k, 1]] + ['{:.9g}'.format(x) for x in rows[k, :19]])
      for row in body_table(bodies, rows, int(nb[e]), poses[e, :, 7].astype(int), masses, gravity):
        wb.writerow(dict(row, step=step))
        print('  body {body:2d} (mesh {mesh:4d}): on [{supports}] under [{carries}]  {points:2d} points  normal load {normal_load:8.4f} N  '
              'held up by {support_up:8.4f} N of {weight:7.4f} N weight: {share:5.2f}'.format(**row))
  print('wrote {} and {}'.format(os.path.join(args.out, 'contacts.csv'), os.path.join(args.out, 'bodies.csv')))
  g.close()


if __name__ == '__main__':
  main()
