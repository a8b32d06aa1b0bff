#!/usr/bin/env python3
"""Time the rock generator: 5,000 rocks on the device (`rocks.generate_pool`: its ten launches between device events — the zero fills of their
output tensors and the host's work between them included, so an upper bound on the kernels' time — and the whole call with its read-back and packing) beside the host's `assets.generate_pool` (timed on `--host-rocks` rocks and scaled),
and one `VecStackEnv.set_pool` of the new pool.  Writes profiles/rocks_generate.txt.

  python tools/bench_rocks.py [--rocks 5000] [--host-rocks 50] [--repeats 5] [--out profiles/rocks_generate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stackrl_amd import assets, rocks  # noqa: E402
from stackrl_amd import env as envs  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rocks', type=int, default=5000)
  ap.add_argument('--host-rocks', type=int, default=50)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rocks_generate.txt'))
  args = ap.parse_args()
  n = args.rocks
  lines = ['rock generator: {} rocks, ten families of irregularity 0.50 .. 0.95, seed 11 ({})'.format(n, torch.cuda.get_device_name(0))]

  rocks.generate(64, 0.5, seed=1)                       # load the library, warm the device
  torch.cuda.synchronize()
  per = n // 10
  kernel_ms = []
  for _ in range(args.repeats):                         # the ten launches of a pool with the fills of their outputs, device events around them
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    batches = [rocks.generate(per, 0.5 + 0.05 * k, seed=11, first_index=k * per, return_points=True) for k in range(10)]
    stop.record()
    torch.cuda.synchronize()
    kernel_ms.append(start.elapsed_time(stop))
  status = torch.cat([b.status for b in batches]).cpu().numpy()
  lines.append('device, ten launches with the zero fills of their outputs (device events, {} repeats; an upper bound on the kernels): median {:.3f} ms, min {:.3f} ms = {:.2f} us per rock; status: {} ok, {} overflow, {} degenerate'.format(
    args.repeats, float(np.median(kernel_ms)), min(kernel_ms), 1e3 * float(np.median(kernel_ms)) / n,
    int((status == 0).sum()), int((status == 1).sum()), int((status == 2).sum())))
  whole = []
  for _ in range(max(1, args.repeats // 2)):
    t0 = time.perf_counter()
    pool = rocks.generate_pool(n, seed=11)
    whole.append(time.perf_counter() - t0)
  lines.append('device, rocks.generate_pool (launches, read-back, packing into a MeshPool): median {:.3f} s'.format(float(np.median(whole))))

  t0 = time.perf_counter()
  assets.generate_pool(args.host_rocks, seed=11)
  host = (time.perf_counter() - t0) / args.host_rocks
  lines.append('host, assets.generate_pool on {} rocks: {:.2f} ms per rock = {:.1f} s per {} rocks'.format(args.host_rocks, 1e3 * host, host * n, n))
  lines.append('ratio host / device (whole call): {:.0f}x; host / launches: {:.0f}x'.format(host * n / float(np.median(whole)),
                                                                                       host * n / (1e-3 * float(np.median(kernel_ms)))))

  e = envs.VecStackEnv(n_parallel=64, seed=11, pool=assets.default_pool(), block=True, episode_length=8)
  e.reset()
  t0 = time.perf_counter()
  e.set_pool(pool)
  set_s = time.perf_counter() - t0
  e.reset()
  e.step(e.sample())
  e.close()
  lines.append('VecStackEnv.set_pool of the {} rocks (host preprocessing, upload, object maps): {:.3f} s'.format(n, set_s))

  text = '\n'.join(lines) + '\n'
  print(text, end='')
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
