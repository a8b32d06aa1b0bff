#!/usr/bin/env python3
"""Heuristic baselines on Stack-v2 observations, timed two ways in one process at 1,024 envs x 8 orientations (128 / 32):

  rows         `Baseline(method, goal=True, minorder=1)` on the grouped observation (include/stackrl_baseline_rows.h)
  composition  what the parent commit offered: `expand_orientations` (the overhead map copied G times), `heuristic_values`
               and `select` per expanded sample, then the row choice in torch

Both give the same actions (checked before timing).  Prints one JSON line per method: the median and the spread
(max - min) of `--repeats` timed runs of each, in milliseconds."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stackrl_amd import baselines, policies   # noqa: E402


def observations(B, G, H, h, seed=0):
  rng = np.random.RandomState(seed)
  m = np.zeros((B, H, H, 2), np.uint8)
  m[..., 0] = rng.randint(0, 90, (B, H, H)) * (rng.rand(B, H, H) < 0.5)
  m[:, H // 8:H // 8 + H // 2, H // 8:H // 8 + H // 2, 1] = 170
  o = (rng.randint(1, 120, (B, G, h, h, 1)) * (rng.rand(B, G, h, h, 1) < 0.6)).astype(np.uint8)
  return torch.from_numpy(m).cuda(), torch.from_numpy(o).cuda()


def composition(method, inputs, minorder):
  xm, xo = inputs
  B, G = xo.shape[0], xo.shape[1]
  em, eo = policies.expand_orientations(inputs)
  vals, mask = baselines.heuristic_values(method, (em.contiguous(), eo.contiguous()))
  a, neg = baselines.select(vals, mask, goal=True, minorder=minorder, value=True)
  A = vals.shape[1] * vals.shape[2]
  c = neg.reshape(B * G, A).gather(1, a[:, None]).reshape(B, G)
  row = torch.argmax(c, dim=1)
  return row * A + a.reshape(B, G).gather(1, row[:, None])[:, 0]


def timed(fn, repeats, warmup):
  for _ in range(warmup):
    fn()
  out = []
  for _ in range(repeats):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); fn(); t1.record()
    torch.cuda.synchronize()
    out.append(t0.elapsed_time(t1))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=1024)
  ap.add_argument('--rows', type=int, default=8)
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  args = ap.parse_args()
  inputs = observations(args.envs, args.rows, 128, 32)
  for method in ('height', 'difference'):
    pol = baselines.Baseline(method, goal=True, minorder=1)
    assert torch.equal(pol(inputs), composition(method, inputs, 1)), method
    rows = timed(lambda: pol(inputs), args.repeats, args.warmup)
    comp = timed(lambda: composition(method, inputs, 1), args.repeats, args.warmup)
    print(json.dumps({'method': method, 'envs': args.envs, 'rows': args.rows, 'repeats': args.repeats,
                      'rows_ms': round(statistics.median(rows), 3), 'rows_spread_ms': round(max(rows) - min(rows), 3),
                      'composition_ms': round(statistics.median(comp), 3),
                      'composition_spread_ms': round(max(comp) - min(comp), 3)}), flush=True)


if __name__ == '__main__':
  main()
