#!/usr/bin/env python3
"""Time of one step of the policy-comparison statistics (include/stackrl_compare.h) on the device: the kernel of
csrc/compare.hip (k_compare and k_fold, through `MapStatistics.step`) against the same definition composed from torch ops
(batched matrix products for the P x P sums and counts), alternating within one run; device events around every launch, the median
and the mean over `--launches` launches after a warm-up.

  python tools/bench_compare.py [--launches 200] [--envs 1024] [--actions 9409] [--out profiles/compare_stats.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stackrl_amd import compare  # noqa: E402


def torch_step(values, record, A):
  """The definition in torch ops on the device: one record's worth of sums and counts added to `record`; returns amax."""
  x32 = torch.stack([v.float() for v in values])
  P, B = x32.shape[:2]
  x = x32.double()
  s = x.sum(-1)
  mu = (s / A)[..., None]
  sigma = torch.sqrt(((x - mu) ** 2).sum(-1) / A)[..., None]
  def gram(t):                                   # sum over envs of the P x P products of an env's maps (a batch of B products)
    t = t.permute(1, 0, 2)
    return torch.bmm(t, t.transpose(1, 2)).sum(0)
  i, j = torch.triu_indices(P, P, device=x.device)
  rec = [torch.full((1,), float(B), dtype=torch.float64, device=x.device), s.sum(-1), gram(x)[i, j]]
  for f in ((x > mu).double(), (x > mu + sigma).double()):
    inter = gram(f)
    n = torch.diagonal(inter)
    rec += [inter[i, j], (n[:, None] + n[None] - inter)[i, j]]
  record += torch.cat(rec)
  return x32.amax(-1)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--launches', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--envs', type=int, default=1024)
  ap.add_argument('--actions', type=int, default=9409)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_compare needs a HIP device')
  B, A = args.envs, args.actions
  lines = ['policy-comparison statistics, one step: B = {}, A = {}, {} launches each after {} warm-ups, alternating; {}'.format(
    B, A, args.launches, args.warmup, torch.cuda.get_device_name(0)),
    '{:>2} {:>8} {:>12} {:>12} {:>12} {:>10} {:>12} {:>12} {:>10}'.format(
      'P', 'inputs', 'bytes', 'kernel ms', '(mean)', 'GB/s', 'torch ms', '(mean)', 'GB/s')]
  print('\n'.join(lines), flush=True)
  for P in (5, 8):
    for dtype in (torch.float32, torch.float64):
      g = torch.Generator(device='cuda').manual_seed(P)
      values = [torch.randn((B, A), generator=g, device='cuda', dtype=dtype) * (1 + j) for j in range(P)]
      st = compare.MapStatistics(P, A, 'cuda')
      rec = torch.zeros(st.R, dtype=torch.float64, device='cuda')
      st.step(values)
      torch_step(values, rec, A)
      torch.cuda.synchronize()
      err = float(((st.record - rec).abs() / rec.abs().clamp(min=1)).max())
      t = {'kernel': [], 'torch': []}
      for k in range(args.warmup + args.launches):
        for name, fn in (('kernel', lambda: st.step(values)), ('torch', lambda: torch_step(values, rec, A))):
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          fn()
          e1.record()
          e1.synchronize()
          if k >= args.warmup:
            t[name].append(e0.elapsed_time(e1))
      nbytes = P * B * A * values[0].element_size()
      med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
      mean = {k: sum(v) / len(v) for k, v in t.items()}
      lines.append('{:>2} {:>8} {:>12} {:>12.4f} {:>12.4f} {:>10.1f} {:>12.4f} {:>12.4f} {:>10.1f}   (records agree to {:.1e} relative)'.format(
        P, str(dtype).replace('torch.', ''), nbytes, med['kernel'], mean['kernel'], nbytes / med['kernel'] / 1e6, med['torch'],
        mean['torch'], nbytes / med['torch'] / 1e6, err))
      print(lines[-1], flush=True)
  lines.append('bytes: the algorithmic bytes P * B * A * element size, read once; GB/s = bytes / median time; the kernel time '
               'includes k_fold and the launch of both kernels')
  print(lines[-1], flush=True)
  text = '\n'.join(lines)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
