#!/usr/bin/env python3
"""Measure the push test (csrc/push.hip, stackrl_amd/push.py) on piles an env has built.  Three parts, all written to
profiles/push_test.txt; no number is aimed at, whatever comes out is reported.

  hooks    the device route — `poses()`, `kick()`, `distances(since=...)`: three launches, between one pair of device events —
           beside the only other route to the same numbers, the blocking host hooks: `velocities()` (srl_get_velocities), a
           numpy add, `set_body_state` (srl_set_body_state), `state()` (srl_get_state) and the numpy restatement of the rows
           and the summary (tests/push_cases.py) on --host-envs envs, scaled to the batch.  1,024 envs x 8 rocks and
           2,048 x 32.  The increment is zero, so every repetition sees the same piles; the two routes are compared bit for bit
           on the envs restated.
  push     one `PushTest.evaluate` at 128 envs x 8 trials x 8 rocks (fork, kick, --substeps sub-steps, distances), by the wall
           clock around a synchronised call.
  policy   `height`, `height+look8` and `height+look8` with a push and a penalty in its score (tools/push_test.py): mean return
           and mean moved / nb of one batch of episodes, seed 11, 128 envs x 8 rocks.

  python tools/bench_push.py [--iters 20] [--host-envs 16] [--substeps 50] [--speed 0.1] [--penalty 0.5 2.0] [--out profiles/push_test.txt]
                             [--quick]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_contacts import build_pile, clocks   # noqa: E402 (the piles and the clock line of the contact benchmark)

CONFIGS = ((1024, 8), (2048, 32))
TOL = (1e-3, 1e-2)


def time_device(g, dv, iters):
  from stackrl_amd import push
  B, L = g.batch_size, g.config.episode_length
  ref = (torch.empty((B, L, 8), dtype=torch.float32, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda'))
  out = push.empty(B, L, g._device, g.config.velocity_threshold)

  def route():
    g.poses(out=ref)
    g.kick(dv)
    return g.distances(since=ref, tol=TOL, out=out)
  for _ in range(3):
    route()
  torch.cuda.synchronize()
  us = []
  for _ in range(iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    route()
    b.record()
    b.synchronize()
    us.append(a.elapsed_time(b) * 1e3)
  return out, us


def time_host(g, dv, host_envs):
  import push_cases as pc
  L = g.config.episode_length
  before, nb0, _, _ = g.state()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  v = g.velocities()
  v[:, :L] = v[:, :L] + dv
  g.set_body_state(None, v)
  poses, nb, _, _ = g.state()
  t1 = time.perf_counter()
  restated = [pc.rows_summary(poses[e, :L], v[e, :L], nb[e], before[e, :L, :7], ref=before[e, :L], ref_nb=nb0[e], tol=TOL) for e in range(host_envs)]
  t2 = time.perf_counter()
  return (t1 - t0) * 1e6, (t2 - t1) * 1e6 / host_envs * g.batch_size, restated


def hooks(lines, args):
  import push_cases as pc
  for n, L in (((64, 8),) if args.quick else CONFIGS):
    g = build_pile(n, L)
    dv = torch.zeros((n, L, 8), dtype=torch.float32, device='cuda')
    out, us = time_device(g, dv, args.iters)
    copy_us, restate_us, restated = time_host(g, dv.cpu().numpy(), min(args.host_envs, n))
    d = out.cpu()
    same = all(pc.same_bits(d.rows[e].numpy(), r) and pc.same_bits(d.summary[e].numpy(), s) for e, (r, s) in enumerate(restated))
    lines.append('{} envs x {} rocks: poses [{}, {}, 8] + kick [{}, {}, 8] + distances rows [{}, {}, 4], summary [{}, 8]'.format(n, L, n, L, n, L, n, L, n))
    lines.append('  device route  {:10.1f} us ({:.1f} .. {:.1f}): three launches between one pair of device events'.format(
      statistics.median(us), min(us), max(us)))
    lines.append('  host route    {:10.1f} us = get_velocities + add + set_body_state + get_state {:.1f} us + restatement {:.1f} us for the batch; '
                 'the two routes agree bit for bit on {} envs: {}'.format(copy_us + restate_us, copy_us, restate_us, len(restated), same))
    g.close()


def one_push(lines, args):
  from stackrl_amd import env as envs
  from stackrl_amd.push import PushSpec, PushTest
  n, k, L = (16, 2, 8) if args.quick else (128, 8, 8)
  g = envs.VecStackEnv(n_parallel=n, seed=11, block=True, episode_length=L)
  g.reset()
  aw = g.config.overhead_res - g.config.object_res + 1
  for _ in range(L):
    a = g.sample()
    a[::2] = (aw // 2) * aw + aw // 2
    g.step(a)
  tester = PushTest(g, trials=k)
  spec = PushSpec(speed=args.speed, substeps=args.substeps, mode='bump', seed=11)
  ms = []
  for it in range(2 + 5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = tester.evaluate(spec)
    torch.cuda.synchronize()
    if it >= 2:
      ms.append((time.perf_counter() - t0) * 1e3)
  lines.append('PushTest.evaluate, {} envs x {} trials x {} rocks (piles full), bump at {} m/s, {} sub-steps: {:.2f} ms ({:.2f} .. {:.2f}), wall '
               'clock around a synchronised call, 5 calls after 2; mean moved / nb {:.4f}, at rest afterwards {:.3f} of the forks'.format(
                 n, k, L, args.speed, args.substeps, statistics.median(ms), min(ms), max(ms), float(d.moved_fraction.mean()),
                 float(d.at_rest.float().mean())))
  tester.close(); g.close()


def policies(lines, args):
  import push_test
  from stackrl_amd import env as envs
  from stackrl_amd.push import PushSpec, PushTest
  n, L, K, trials = (16, 4, 4, 2) if args.quick else (128, 8, 8, 4)
  spec = PushSpec(speed=args.speed, substeps=args.substeps, mode='bump', seed=11)
  lines.append('policies, one batch of episodes each, seed 11, {} envs x {} rocks; after every step {} bump trials at {} m/s, {} sub-steps, '
               'on forks; moved: beyond {:.4g} m or {:.4g} rad'.format(n, L, trials, args.speed, args.substeps, *push_test_tol(spec, n, L)))
  lines.append('  {:28s} {:>12s} {:>16s} {:>10s}'.format('policy', 'mean return', 'mean moved / nb', 'seconds'))
  for look_k, penalty in [(0, 0.0), (K, 0.0)] + [(K, p) for p in args.penalty]:
    g = envs.VecStackEnv(n_parallel=n, seed=11, block=True, episode_length=L)
    tester = PushTest(g, trials=trials)
    policy, look = push_test.make_policy(g, 'height', look_k, spec, penalty, 11)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ret, share = push_test.run_episode(g, policy, tester, spec)
    torch.cuda.synchronize()
    lines.append('  {:28s} {:12.4f} {:16.4f} {:10.2f}'.format(push_test.label('height', look_k, penalty), ret, share, time.perf_counter() - t0))
    for x in (look, tester, g):
      if x is not None:
        x.close()


def push_test_tol(spec, n, L):
  from stackrl_amd.config import StackConfig
  from stackrl_amd.push import default_tol
  return spec.tol or default_tol(StackConfig(n_envs=n, episode_length=L))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--host-envs', type=int, default=16)
  ap.add_argument('--substeps', type=int, default=50)
  ap.add_argument('--speed', type=float, default=0.1)
  ap.add_argument('--penalty', type=float, nargs='+', default=[0.5, 2.0])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'push_test.txt'))
  ap.add_argument('--quick', action='store_true', help='small shapes only (a smoke run of the tool)')
  args = ap.parse_args()
  lines = ['push test (srl_k_poses, srl_k_kick, srl_k_pose_distances; PushTest; the lookahead with a push); ' + torch.cuda.get_device_name(0),
           'clocks as found before the first launch, nothing set: ' + clocks(),
           'hooks: median (min .. max) of {} repetitions after 3; host: the blocking hooks on the batch, and the numpy restatement on {} envs '
           'scaled to the batch'.format(args.iters, args.host_envs)]
  hooks(lines, args)
  one_push(lines, args)
  policies(lines, args)
  lines.append('clocks right after the last launch: ' + clocks())
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
