#!/usr/bin/env python3
"""What picking the candidates of a lookahead costs (csrc/candidates.hip), and what spreading them buys.

  (a) `candidates.select` (one launch of k_candidates) at k = 8 on 128, 1,024 and 4,096 envs x one 97 x 97 float32 map and on
      1,024 envs x 8 maps: at radius 0 beside `lookahead.candidates` (two stable `torch.sort`s), which gives the same result,
      and at radius 4 beside `candidates.select_reference` (k rounds of arg-max and masking in torch), which gives the same
      result.  The results are compared before anything is timed.  The maps are smooth (a bump per map plus noise), as a
      policy's are.
  (b) the return table of `compare.run` at seed 11, 128 envs x 8 rocks, 256 steps per policy — the setting of
      profiles/state_lookahead.txt — for `height`, `height+look8` and `height+look8r{1,2,4,8,16}`, and how many distinct
      candidates an env had on average at each radius.

Every time is the median of `--runs` runs (at least 20), each timed with events on the stream after separate warm-up launches.

  python tools/bench_candidates.py [--runs 25] [--steps 256] [--skip-returns] [--out profiles/lookahead_candidates.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OH, K = 97, 8
RADII = (1, 2, 4, 8, 16)


def median_us(fn, runs):
  """Median microseconds of `fn()` over `runs` runs, each between two events."""
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3)
  return statistics.median(times)


def smooth_maps(B, G, seed):
  gen = torch.Generator(device='cuda').manual_seed(seed)
  y = torch.linspace(0, 1, OH, device='cuda')[:, None]
  x = torch.linspace(0, 1, OH, device='cuda')[None, :]
  c = torch.rand(B, G, 2, 1, 1, generator=gen, device='cuda')
  v = -((y - c[:, :, 0]) ** 2 + (x - c[:, :, 1]) ** 2) + 1e-3 * torch.randn(B, G, OH, OH, generator=gen, device='cuda')
  return v.reshape(B, G * OH * OH).contiguous()


def timing_lines(runs):
  from stackrl_amd import candidates, lookahead
  lines = ['candidates.select at k = {}, {} x {} float32 maps: kernel beside the torch composition that gives the same result'.format(K, OH, OH)]
  for B, G in ((128, 1), (1024, 1), (4096, 1), (1024, 8)):
    values = smooth_maps(B, G, B + G)
    action = values.argmax(dim=1)
    nbytes = values.numel() * 4
    for radius, name, other in ((0, 'lookahead.candidates', lambda: lookahead.candidates(action, values, K, G, OH * OH)),
                                (4, 'select_reference', lambda: candidates.select_reference(values, action, k=K, radius=4, OH=OH)[0])):
      kernel = lambda: candidates.select(values, action, k=K, radius=radius, OH=OH)      # noqa: E731
      if not torch.equal(kernel()[0], other()):
        raise SystemExit('the kernel and {} disagree at {} envs x {} maps, radius {}'.format(name, B, G, radius))
      us, us_other = median_us(kernel, runs), median_us(other, runs)
      lines.append('  {:>5,} envs x {} map{} radius {}   kernel {:9.1f} us ({:5.2f} TB/s of values read once)   {:<20} {:10.1f} us   kernel / torch = {:.4f}'.format(
        B, G, 's' if G > 1 else ' ', radius, us, nbytes / us / 1e6, name, us_other, us / us_other))
    del values, action
    torch.cuda.empty_cache()
  return lines


class Counted(object):
  """A `LookaheadPolicy` that also sums `last_count`."""

  def __init__(self, policy):
    self.policy, self.total, self.calls = policy, 0.0, 0

  def __call__(self, obs, n_valid=None):
    out = self.policy(obs, n_valid=n_valid) if n_valid is not None else self.policy(obs)
    if self.policy.last_count is not None:
      self.total += float(self.policy.last_count.float().mean())
      self.calls += 1
    return out


def return_lines(steps, B=128, L=8, seed=11):
  from stackrl_amd import compare
  from stackrl_amd import env as envs
  from stackrl_amd.baselines import Baseline
  from stackrl_amd.lookahead import Lookahead, LookaheadPolicy
  env = envs.VecStackEnv(n_parallel=B, seed=seed, block=True, episode_length=L)
  look = Lookahead(env, K)
  height = Baseline('height', value=True)
  policies = {'height': height, 'height+look{}'.format(K): LookaheadPolicy(height, look)}
  for r in RADII:
    policies['height+look{}r{}'.format(K, r)] = Counted(LookaheadPolicy(height, look, radius=r))
  res = compare.analyse(compare.run(env, policies, num_steps=steps, seed=seed))
  look.close(); env.close()
  lines = ['compare.run at seed {}, {} envs x {} rocks, {} steps per policy: episode returns (mean +/- standard error)'.format(seed, B, L, steps)]
  for name, r, sd in zip(res['keys'], res['return'], res['return_std']):
    p = policies[str(name)]
    extra = '   distinct candidates per env and step {:.2f} of {}'.format(p.total / p.calls, K) if isinstance(p, Counted) and p.calls else ''
    lines.append('  {:<18} {:8.4f} +/- {:.4f}{}'.format(str(name), r, sd, extra))
  return lines


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=25)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--skip-returns', action='store_true')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lookahead_candidates.txt'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_candidates needs a HIP device')
  if args.runs < 20:
    raise SystemExit('--runs must be at least 20 (the figures are medians)')
  lines = ['lookahead candidates; {}; medians of {} runs, events on the stream'.format(torch.cuda.get_device_name(0), args.runs)]
  lines += timing_lines(args.runs)
  if not args.skip_returns:
    lines += return_lines(args.steps)
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
