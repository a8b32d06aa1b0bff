#!/usr/bin/env python3
"""Generate rock models on the device: the reference's `generate` command (`python -m stackrl generate`;
stackrl/envs/data/generator.py) through `stackrl_amd.rocks`.  Writes `<irregularity>_<index>.obj` / `.urdf` and `log.csv` into
the directory (`MeshPool.write_directory`), which `assets.load_directory` and the reference's env read.

  python tools/generate_rocks.py [-n 100] [-d DIR] [--seed S] [-i 0.5 ...] [--irregularity-range START:STOP:STEP] [--split]
                                 [--subdivisions 3] [--extents 1,0.5,0.333] [--fit 0]

`-n` rocks per irregularity; without `-i` / `--irregularity-range` the irregularities are 0.05 ... 1.00.  `--split` writes each
irregularity into its own sub-directory `DIR/<irregularity>`.  A rock the kernel does not report ok (none in 5,000 so far) is
finished on the host from its own points.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stackrl_amd import assets, rocks  # noqa: E402


def irregularities(args):
  out = list(args.irregularity or [])
  if args.irregularity_range:
    start, stop, step = (float(x) for x in args.irregularity_range.split(':'))
    k = 0
    while start + k * step < stop - 1e-9:
      out.append(round(start + k * step, 6))
      k += 1
  return out or [i / 100. for i in range(5, 101, 5)]


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
  ap.add_argument('-n', type=int, default=100, help='rocks per irregularity')
  ap.add_argument('-d', '--directory', default=os.path.join('.', 'generated'))
  ap.add_argument('--seed', type=int, default=None)
  ap.add_argument('-i', '--irregularity', type=float, action='append')
  ap.add_argument('--irregularity-range', metavar='START:STOP:STEP')
  ap.add_argument('--split', action='store_true')
  ap.add_argument('--subdivisions', type=int, default=3)
  ap.add_argument('--extents', default='1,0.5,0.3333333333333333')
  ap.add_argument('--fit', type=int, default=0, choices=(0, 1),
                  help='0: bounding sphere about the centre of mass (the shipped pool); 1: longest box extent (generator.py:114-116)')
  args = ap.parse_args()
  irrs = irregularities(args)
  extents = tuple(float(x) for x in args.extents.split(','))
  if len(extents) != 3:
    ap.error('--extents takes three numbers')
  seed = args.seed if args.seed is not None else int.from_bytes(os.urandom(4), 'little')
  digits = len(str(max(args.n - 1, 1)))
  t0 = time.time()
  batches = [rocks.generate(args.n, irr, seed=seed, first_index=k * args.n, subdivisions=args.subdivisions, extents=extents,
                            fit=args.fit, return_points=True) for k, irr in enumerate(irrs)]
  pools = []
  for irr, b in zip(irrs, batches):
    names = ['{}_{:0{}d}'.format(int(round(irr * 100)), i, digits) for i in range(args.n)]
    pools.append((irr, b.to_pool(names), int((b.status != 0).sum())))
  t1 = time.time()
  if args.split:
    for irr, pool, _ in pools:
      pool.write_directory(os.path.join(args.directory, str(int(round(irr * 100)))))
  else:
    assets.pack([pool.mesh(i) for _, pool, _ in pools for i in range(len(pool))],
                [n for _, pool, _ in pools for n in pool.names]).write_directory(args.directory)
  print('{} rocks ({} irregularities x {}) with seed {}: made in {:.3f} s ({} finished on the host), written to {} in {:.1f} s'.format(
    len(irrs) * args.n, len(irrs), args.n, seed, t1 - t0, sum(f for _, _, f in pools), args.directory, time.time() - t1))


if __name__ == '__main__':
  main()
