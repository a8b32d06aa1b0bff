#!/usr/bin/env python3
"""What saving, restoring and forking env states costs (csrc/state.hip), and what a one-step lookahead buys.

  (a) `srl_state_get` / `srl_state_set` at 1,024 envs x 8 rocks and 4,096 x 16, and `set` forked 8-fold (128 records into
      1,024 envs) at the first shape: microseconds and the bytes of records moved per second, beside `torch.index_select` /
      `index_copy_` moving the same bytes through [n, words] int32 tensors.  (A record copied is read once and written once:
      the memory traffic is twice the figure.)
  (b) `Lookahead.evaluate` with k = 8 at 128 envs x 8 rocks, split into its get, set and step, beside a plain `step` of a
      1,024-env handle restored to the same point of its episode before every run.
  (c) the return table of `compare.run` for `height`, `height+look8` and `random` at seed 11, 128 envs, 256 steps.

Every time is the median of `--runs` runs (at least 20), each timed with events on the stream after separate warm-up launches.

  python tools/bench_lookahead.py [--runs 25] [--steps 256] [--skip-returns] [--out profiles/state_lookahead.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_us(fn, runs, before=None):
  """Median microseconds of `fn()` over `runs` runs, each between two events; `before()` runs untimed ahead of each."""
  for _ in range(3):
    if before:
      before()
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(runs):
    if before:
      before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3)
  return statistics.median(times)


def mid_episode(envs, n, L, placed, **kw):
  env = envs.VecStackEnv(n_parallel=n, seed=11, block=True, episode_length=L, **kw)
  env.reset()
  for _ in range(placed):
    env.step(env.sample())
  return env


def copy_lines(envs, n, L, runs, fork=None):
  """get and set of n envs x L rocks (and with `fork` = (records, fold) the forked set) beside the torch copies."""
  from stackrl_amd import env as _e
  env = mid_episode(envs, n, L, L // 2)
  rec, _, _ = env._get_records()
  words = rec.shape[1]
  sig = env.state_signature()
  stream = lambda: env._stream()      # noqa: E731
  nbytes = n * words * 4
  table = torch.empty_like(rec).copy_(rec)          # the comparator's "handle": the same bytes as one [n, words] tensor
  out = torch.empty_like(rec)
  idx32 = torch.arange(n, dtype=torch.int32, device=rec.device)
  idx64 = idx32.to(torch.int64)

  def get():
    _e._check(env._lib.srl_state_get(env._h, idx32.data_ptr(), n, out.data_ptr(), None, None, stream()))

  def set_():
    _e._check(env._lib.srl_state_set(env._h, ctypes.c_uint64(sig), idx32.data_ptr(), idx32.data_ptr(), n, rec.data_ptr(), stream()))

  rows = [('get', median_us(get, runs), median_us(lambda: torch.index_select(table, 0, idx64, out=out), runs), nbytes),
          ('set', median_us(set_, runs), median_us(lambda: table.index_copy_(0, idx64, rec), runs), nbytes)]
  assert torch.equal(out, rec)
  if fork:
    m, fold = fork
    src32 = torch.arange(m, dtype=torch.int32, device=rec.device).repeat_interleave(fold)
    src64 = src32.to(torch.int64)
    few = rec[:m].contiguous()

    def forked():
      _e._check(env._lib.srl_state_set(env._h, ctypes.c_uint64(sig), None, src32.data_ptr(), m * fold, few.data_ptr(), stream()))
    rows.append(('set, {} records {}-fold'.format(m, fold), median_us(forked, runs),
                 median_us(lambda: torch.index_select(few, 0, src64, out=table), runs), m * fold * words * 4))
  env.close()
  lines = ['{:,} envs x {} rocks: {:,} words = {:.1f} KB per record, {:.1f} MB per batch'.format(n, L, words, words * 4 / 1e3, nbytes / 1e6)]
  for name, us, us_torch, b in rows:
    lines.append('  {:<28} kernel {:9.1f} us  {:6.2f} TB/s of records   torch {:9.1f} us  {:6.2f} TB/s   kernel / torch = {:.2f}'.format(
      name, us, b / us / 1e6, us_torch, b / us_torch / 1e6, us / us_torch))
  return lines


def evaluate_lines(envs, runs, B=128, k=8, L=8):
  from stackrl_amd.lookahead import Lookahead
  env = mid_episode(envs, B, L, L // 2)
  look = Lookahead(env, k)
  s = look.scratch
  gen = torch.Generator().manual_seed(1)
  cand = torch.randint(0, env.n_actions, (B, k), generator=gen).cuda()
  flat = cand.reshape(-1)
  state = {}

  def get():
    state['rec'] = env._get_records()[0]

  def set_():
    s._set_records(state['rec'], look.signature, None, look._source)
    s._left = env._left

  us_get = median_us(get, runs)
  us_set = median_us(set_, runs)
  us_step = median_us(lambda: s.step(flat, block=True), runs, before=set_)
  us_all = median_us(lambda: look.evaluate(cand), runs)
  plain = mid_episode(envs, B * k, L, L // 2)
  snap = plain.get_state()
  acts = torch.randint(0, plain.n_actions, (B * k,), generator=gen).cuda()
  us_plain = median_us(lambda: plain.step(acts, block=True), runs, before=lambda: plain.set_state(snap))
  look.close(); env.close(); plain.close()
  return ['Lookahead.evaluate, k = {} at {} envs x {} rocks ({} of {} placed): {:,} scratch envs'.format(k, B, L, L // 2, L, B * k),
          '  evaluate                {:9.1f} us'.format(us_all),
          '    get  ({} records)    {:9.1f} us'.format(B, us_get),
          '    set  ({}-fold)         {:9.1f} us'.format(k, us_set),
          '    step ({:,} envs)    {:9.1f} us'.format(B * k, us_step),
          '  plain step of a {:,}-env handle at the same point of its episode   {:9.1f} us'.format(B * k, us_plain),
          '  the two copies are {:.2f} % of the evaluate; evaluate / plain step = {:.3f}'.format(100 * (us_get + us_set) / us_all, us_all / us_plain)]


def return_lines(envs, steps, B=128, k=8, L=8, seed=11):
  from stackrl_amd import compare
  from stackrl_amd.baselines import Baseline
  from stackrl_amd.lookahead import Lookahead, LookaheadPolicy
  env = envs.VecStackEnv(n_parallel=B, seed=seed, block=True, episode_length=L)
  look = Lookahead(env, k)
  height = Baseline('height', value=True)
  policies = {'height': height, 'height+look{}'.format(k): LookaheadPolicy(height, look), 'random': Baseline('random', value=True, seed=3)}
  res = compare.analyse(compare.run(env, policies, num_steps=steps, seed=seed))
  look.close(); env.close()
  lines = ['compare.run at seed {}, {} envs x {} rocks, {} steps per policy: episode returns'.format(seed, B, L, steps)]
  for name, r, sd in zip(res['keys'], res['return'], res['return_std']):
    lines.append('  {:<14} {:8.4f} +/- {:.4f}'.format(name, r, sd))
  return lines


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=25)
  ap.add_argument('--steps', type=int, default=256)
  ap.add_argument('--skip-returns', action='store_true')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'state_lookahead.txt'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_lookahead needs a HIP device')
  if args.runs < 20:
    raise SystemExit('--runs must be at least 20 (the figures are medians)')
  from stackrl_amd import env as envs
  lines = ['state records and one-step lookahead; {}; medians of {} runs, events on the stream'.format(torch.cuda.get_device_name(0), args.runs)]
  lines += copy_lines(envs, 1024, 8, args.runs, fork=(128, 8))
  lines += copy_lines(envs, 4096, 16, args.runs)
  lines += evaluate_lines(envs, args.runs)
  if not args.skip_returns:
    lines += return_lines(envs, args.steps)
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
