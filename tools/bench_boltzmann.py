#!/usr/bin/env python3
"""Boltzmann exploration on the rollout path: (a) `k_boltzmann_head` beside `k_policy_head`, (b) `DQN.policy(exploration=True)`
per batch in both exploration modes (`FusedPolicy(fast=True)`, xcorr='bf16x3').  Device events around timed repeats after a
warm-up; one JSON line per figure.

  bench_boltzmann.py [B] [heads] [epsilon-greedy] [boltzmann]      (default: B = 4096, all three legs)"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stackrl_amd import nets, qops
from stackrl_amd.dqn import DQN

args = sys.argv[1:]
B = int(args.pop(0)) if args and args[0].isdigit() else 4096
legs = args or ['heads', 'epsilon-greedy', 'boltzmann']
A = 9409
g = torch.Generator(device='cuda').manual_seed(0)


def timed(f, warmup, repeats):
  """Median and extremes of `repeats` single calls, each between two device events (ms)."""
  for _ in range(warmup):
    f()
  torch.cuda.synchronize()
  ts = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record()
    b.synchronize()
    ts.append(a.elapsed_time(b))
  ts.sort()
  return {'median_ms': round(ts[len(ts) // 2], 4), 'min_ms': round(ts[0], 4), 'max_ms': round(ts[-1], 4), 'repeats': repeats}


def report(what, **kw):
  print(json.dumps(dict(what=what, B=B, **kw)), flush=True)


if 'heads' in legs:
  adv = 3 * torch.randn((B, A), generator=g, device='cuda')
  u = torch.rand(B, generator=g, device='cuda')
  rnd = torch.randint(A, (B,), generator=g, device='cuda')
  keys = torch.randint(0, 2 ** 32, (B, 2), dtype=torch.int64, generator=g, device='cuda')
  for _ in range(2):          # alternated: the two kernels see the same machine
    report('k_policy_head', A=A, **timed(lambda: qops.policy_head(adv, u, rnd, 0.1), 5, 50))
    report('k_boltzmann_head', A=A, **timed(lambda: qops.boltzmann_head(adv, keys, 0.7), 5, 50))
  del adv

modes = [m for m in legs if m != 'heads']
if modes:
  net = nets.DeepQSiamFCN(seed=1).cuda().eval()
  x = (torch.randint(0, 256, (B, 128, 128, 2), generator=g, device='cuda', dtype=torch.uint8),
       torch.randint(0, 256, (B, 32, 32, 1), generator=g, device='cuda', dtype=torch.uint8))
  chunk = int(os.environ.get('SRL_POLICY_CHUNK', 2048))
  agents = {m: DQN(net, exploration_mode=m, exploration=0.1 if m == 'epsilon-greedy' else 0.7, collect_batch_size=B,
                   replay_memory_size=2 * B, seed=9, policy_op=qops.FusedPolicy(chunk=chunk, fast=True), xcorr='bf16x3') for m in modes}
  for rnd_ in range(2):       # alternated
    for m in modes:
      report('DQN.policy(exploration=True)', mode=m, chunk=chunk, **timed(lambda: agents[m].policy(x, exploration=True), 2 if rnd_ == 0 else 0, 5))
