#!/usr/bin/env python3
"""Greedy acting: `agent.policy(x, values=True)` (the plain torch module and a [B, A] Q tensor: what `Trainer.eval` and the
greedy policies call without `fused_eval`) against `agent.greedy(x, stats=True)` (`FusedPolicy.greedy`: the rollout kernels,
`srl_tvalue_fwd`, `srl_greedy_head`), on (a) B x (128, 32) samples and (b) a Stack-v2 observation of E envs with G = 8
object maps each, where the plain path is `policies.OrientationGreedy` on the expanded observation.  Device events around
single calls after a warm-up, the two paths alternated; one JSON line per figure.

  bench_greedy.py [B] [E]      (default: B = 1024, E = 128)"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stackrl_amd import nets, qops
from stackrl_amd.dqn import DQN
from stackrl_amd.policies import FusedOrientationGreedy, OrientationGreedy

args = sys.argv[1:]
B = int(args[0]) if args else 1024
E = int(args[1]) if len(args) > 1 else 128
G = 8
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
  print(json.dumps(dict(what=what, **kw)), flush=True)


net = nets.DeepQSiamFCN(seed=1).cuda().eval()
chunk = int(os.environ.get('SRL_POLICY_CHUNK', 2048))
agent = DQN(net, collect_batch_size=B, replay_memory_size=2 * B, seed=9, policy_op=qops.FusedPolicy(chunk=chunk, fast=True), xcorr='bf16x3')

adv = 3 * torch.randn((B, 1, net.n_actions), generator=g, device='cuda')
v = torch.randn(B, generator=g, device='cuda')
report('k_greedy_head', B=B, A=net.n_actions, **timed(lambda: qops.greedy_head(adv, v, stats=True), 5, 50))
del adv

x = (torch.randint(0, 256, (B, 128, 128, 2), generator=g, device='cuda', dtype=torch.uint8),
     torch.randint(0, 256, (B, 32, 32, 1), generator=g, device='cuda', dtype=torch.uint8))
for rnd_ in range(2):         # alternated: the two paths see the same machine
  report('agent.policy(values=True)', B=B, **timed(lambda: agent.policy(x, values=True), 2 if rnd_ == 0 else 0, 5))
  report('agent.greedy(stats=True)', B=B, chunk=chunk, **timed(lambda: agent.greedy(x, stats=True), 2 if rnd_ == 0 else 0, 5))
del x

x = (torch.randint(0, 256, (E, 128, 128, 2), generator=g, device='cuda', dtype=torch.uint8),
     torch.randint(0, 256, (E, G, 32, 32, 1), generator=g, device='cuda', dtype=torch.uint8))
plain, fused = OrientationGreedy(agent.q_net, value=True), FusedOrientationGreedy(agent)
for rnd_ in range(2):
  report('OrientationGreedy(value=True)', envs=E, G=G, **timed(lambda: plain(x), 2 if rnd_ == 0 else 0, 5))
  report('FusedOrientationGreedy', envs=E, G=G, chunk=chunk, **timed(lambda: fused(x), 2 if rnd_ == 0 else 0, 5))
