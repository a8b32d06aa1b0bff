#!/usr/bin/env python3
"""Time `contact_points` (csrc/contacts.hip, srl_k_contact_points) on piles an env has built — 1,024 envs x 8 rocks and
2,048 x 32 — beside the only other route to the contact network: the state records copied to the host and decoded there.

  kernel   `env.contact_points(wrench=True, out=...)` of the whole batch: one launch, every launch between its own pair of
           device events after a warm-up, the median over --iters launches; and the same without the wrench
  host     `env.get_state().cpu()` of the whole batch (timed as it is) plus the numpy restatement of the definition
           (tests/contact_cases.py `decode`) on --host-envs envs, scaled to the batch (a loop over envs: linear in them)

Reports both times, the shapes, the contacts found, and whether the two routes agree bit for bit on the envs decoded.  No
ratio is aimed at.  The clocks are left as they are found and named in the output.

  python tools/bench_contacts.py [--iters 20] [--host-envs 16] [--out profiles/contact_points.txt] [--quick]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CONFIGS = ((1024, 8), (2048, 32))


def clocks():
  """The clocks as they are found (nothing is set): what rocm-smi shows, or that it could not be asked."""
  try:
    out = subprocess.run(['rocm-smi', '--showperflevel', '--showclocks', '-d', '0'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                         timeout=20, universal_newlines=True).stdout
    keep = [l.strip() for l in out.splitlines() if 'Performance Level' in l or 'sclk' in l or 'mclk' in l]
    return '; '.join(keep) if keep else 'rocm-smi printed no clock lines'
  except Exception as e:      # noqa: BLE001 (a tool that is missing or hangs must not cost the measurement)
    return 'not read ({})'.format(type(e).__name__)


def build_pile(n, L, seed=11):
  """n envs after L placements: half of them on one pixel (rocks on rocks), the others where `sample` says."""
  from stackrl_amd import env as envs
  g = envs.VecStackEnv(n_parallel=n, seed=seed, block=True, episode_length=L)
  g.reset()
  aw = g.config.overhead_res - g.config.object_res + 1
  centre = (aw // 2) * aw + aw // 2
  for _ in range(L):
    a = g.sample()
    a[::2] = centre
    g.step(a)
  return g


def time_kernel(g, iters, wrench):
  from stackrl_amd import contacts
  out = contacts.empty(g.batch_size, g.contact_max_points(), g.config.episode_length, wrench, g._device)
  for _ in range(3):
    g.contact_points(wrench=wrench, out=out)
  torch.cuda.synchronize()
  us = []
  for _ in range(iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.contact_points(wrench=wrench, out=out)
    b.record()
    b.synchronize()
    us.append(a.elapsed_time(b) * 1e3)
  return out, us


def time_host(g, host_envs, verts):
  import contact_cases as cc
  L, dt = g.config.episode_length, np.float32(g.config.sim_time_step)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  rec = g.get_state().cpu().records.numpy()
  t1 = time.perf_counter()
  decoded = [cc.decode(rec[e], L, dt, verts) for e in range(host_envs)]
  t2 = time.perf_counter()
  return (t1 - t0) * 1e6, (t2 - t1) * 1e6 / host_envs * g.batch_size, decoded


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--host-envs', type=int, default=16)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'contact_points.txt'))
  ap.add_argument('--quick', action='store_true', help='64 envs x 8 rocks only (a smoke run of the tool)')
  args = ap.parse_args()
  import contact_cases as cc
  lines = ['contact_points (srl_k_contact_points: count + bodies + rows, with and without the wrench) of piles the envs built; '
           + torch.cuda.get_device_name(0),
           'clocks as found before the first launch, nothing set: ' + clocks(),
           'kernel: median (min .. max) of {} launches, each between device events, after 3 warm-up launches; host: '
           'get_state().cpu() of the batch, and the numpy restatement on {} envs scaled to the batch'.format(args.iters, args.host_envs)]
  for n, L in (((64, 8),) if args.quick else CONFIGS):
    g = build_pile(n, L)
    verts = cc.com_vertices(g.pool)
    out, us_w = time_kernel(g, args.iters, True)
    _, us = time_kernel(g, args.iters, False)
    copy_us, decode_us, decoded = time_host(g, min(args.host_envs, n), verts)
    cp = out.cpu()
    same = all(int(cp.count[e]) == c and np.array_equal(cp.rows[e, :c].numpy().view(np.int32), r[:c].view(np.int32))
               and np.array_equal(cp.bodies[e, :c].numpy(), b[:c]) and np.array_equal(cp.wrench[e].numpy().view(np.int32), w.view(np.int32))
               for e, (c, b, r, w) in enumerate(decoded))
    med = statistics.median
    lines.append('{} envs x {} rocks: capacity {} rows of {} words per env, {} contacts in all, at most {} in an env, {} of them pair points'.format(
      n, L, cp.capacity, cp.rows.shape[2], int(cp.count.sum()), int(cp.count.max()),
      int(sum(int((cp.bodies[e, :int(cp.count[e]), 1] >= 0).sum()) for e in range(n)))))
    lines.append('  kernel with wrench     {:10.1f} us ({:.1f} .. {:.1f})'.format(med(us_w), min(us_w), max(us_w)))
    lines.append('  kernel without wrench  {:10.1f} us ({:.1f} .. {:.1f})'.format(med(us), min(us), max(us)))
    lines.append('  host route             {:10.1f} us = get_state().cpu() {:.1f} us + restatement {:.1f} us for the batch; the two routes agree bit for bit on {} envs: {}'.format(
      copy_us + decode_us, copy_us, decode_us, len(decoded), same))
    g.close()
  lines.append('clocks right after the last launch: ' + clocks())
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
