#!/usr/bin/env python3
"""Env-only steps at BASELINE configs[1] (1,024 envs x 8 rocks, random policy on device) once per observation dtype
(env.py:24): per-kernel HIP-event times of the render kernel (`srl_set_profiling` / `kernel_times()`, as bench.py's leg A),
its achieved bandwidth over the algorithmic bytes, the HBM roofline fraction and env steps/s.

Algorithmic bytes per env and step: bench.py's `alg_bytes_per_env` with the observation widened to the element size s:
(4 + 2s) res^2 (H float32 + the two observation channels) + (4 + s) r^2 maps (the object map's float32 + its observation)
+ 1,404 B per placed rock.  At s = 1 this is bench.py's formula (asserted below).

  python tools/bench_obs_dtypes.py [--steps K] [--warmup W] [--dtypes uint8,float32,...]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTYPES = ('uint8', 'uint16', 'uint32', 'uint64', 'float16', 'float32', 'float64')
SIZE = {'uint8': 1, 'uint16': 2, 'uint32': 4, 'uint64': 8, 'float16': 2, 'float32': 4, 'float64': 8}


def alg_bytes_per_env(res, r, nb, s, maps=1):
  return (4 + 2 * s) * res * res + (4 + s) * r * r * maps + 1404 * nb


def leg(dtype, B, L, steps, warmup, seed, pool):
  import torch
  from stackrl_amd import env as envs
  env = envs.VecStackEnv(n_parallel=B, seed=seed, pool=pool, block=False, episode_length=L, dtype=dtype)
  assert env.observation_spec[0].dtype == getattr(torch, dtype)
  res, r, s = env.config.overhead_res, env.config.object_res, SIZE[dtype]
  phase = {'k': 0}   # calls since reset(): 1..L placements, L + 1 = the auto-reset

  def do_step():
    out = env.step(env.sample())
    phase['k'] += 1
    if phase['k'] == L + 1:
      phase['k'] = 0
      return out, 0, 0
    return out, B, phase['k']

  env.reset()()
  for _ in range(warmup):
    do_step()
  env._lib.srl_sync_status(env._h, env._stream())
  env.kernel_times()
  env.set_profiling(True)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  placed, alg, last = 0, 0, None
  for _ in range(steps):
    last, p, nb = do_step()
    placed += p
    alg += B * alg_bytes_per_env(res, r, nb, s, env.config.n_object_maps)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  last()                   # raises if any env diverged / an action was invalid
  ms, nl = env.kernel_times()
  env.set_profiling(False)
  env.close()
  render_s = float(ms[1]) / 1e3
  return dict(dtype=dtype, size=s, render_us=1e3 * float(ms[1]) / max(int(nl[1]), 1), launches=int(nl[1]),
              alg_bytes_per_launch=alg / max(int(nl[1]), 1), gbs=alg / render_s / 1e9, steps_per_s=placed / dt,
              settle_ms=float(ms[0]) / max(int(nl[0]), 1))


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=54)
  ap.add_argument('--warmup', type=int, default=9)
  ap.add_argument('--envs', type=int, default=1024)
  ap.add_argument('--rocks', type=int, default=8)
  ap.add_argument('--seed', type=int, default=11)
  ap.add_argument('--dtypes', default=','.join(DTYPES))
  args = ap.parse_args(argv)
  import bench
  for res, r, nb in ((128, 32, 0), (128, 32, 8), (64, 16, 3)):
    assert alg_bytes_per_env(res, r, nb, 1) == bench.alg_bytes_per_env(res, r, nb), 'the s = 1 form must be bench.py\'s'
  from stackrl_amd import assets, build
  pool = assets.default_pool()
  info = build.info(build.LIB)
  print('# render kernel per observation dtype: {} envs x {} rocks, {} timed steps after {} warm-up steps; env library {}'.format(
    args.envs, args.rocks, args.steps, args.warmup, info), flush=True)
  print('# {:8s} {:>2s} {:>11s} {:>9s} {:>10s} {:>13s} {:>13s} {:>9s}'.format(
    'dtype', 's', 'render_us', 'GB/s', 'roofline', 'alg_B/launch', 'env_steps/s', 'settle_ms'), flush=True)
  for dt in args.dtypes.split(','):
    d = leg(dt, args.envs, args.rocks, args.steps, args.warmup, args.seed, pool)
    print('  {:8s} {:2d} {:11.2f} {:9.1f} {:10.4f} {:13.0f} {:13.0f} {:9.3f}'.format(
      dt, d['size'], d['render_us'], d['gbs'], d['gbs'] / bench.HBM_PEAK_GBS, d['alg_bytes_per_launch'], d['steps_per_s'],
      d['settle_ms']), flush=True)


if __name__ == '__main__':
  main()
