#!/usr/bin/env python3
"""`render('rgb_array')` of a batch (csrc/view.hip, srl_k_view) against the two other routes to the same images on the same
box, at 128 x 128 / 32 x 32 maps, float64 and uint8:

  kernel   `env.render(dtype, out=...)`: one launch, timed with device events
  torch    the same function composed of torch operations on device copies of the maps (amax, divide, where, stack; for
           uint8 multiply, add, clamp, cast): what a caller could write if the float maps were exposed as tensors
  numpy    `env.maps()` (a device synchronise + the float maps over PCIe) and the colouring in numpy on the host: the only
           route there was; host wall clock

Reports the time per call, the kernel's achieved store bandwidth (the bytes of both images over its time) beside the
~6.3 TB/s of HBM bandwidth an MI355X sustains, and whether the three routes agree bit for bit.

  python tools/bench_view.py [--envs 1024] [--iters 50] [--out profiles/view_ab.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import view_cases as vc  # noqa: E402  (the numpy restatement of the reference's render)

SUSTAINED_TBS = 6.3


def torch_rgb(m, mask, dtype):
  """env.py:299-305 in torch: m float32 [B, H, W], mask bool [B, H, W] or None -> [B, H, W, 3]."""
  mx = m.amax((1, 2), keepdim=True)
  r = torch.where(mx != 0, m / mx, m)
  b = 1 - r
  g = torch.full(m.shape, 0.5, dtype=torch.float64, device=m.device)
  if mask is not None:
    g = g + 0.1 * mask.double()
  x = torch.stack([r.double(), g, b.double()], -1)
  return x if dtype is None else (x * 255 + 0.5).clamp(0, 255).to(torch.uint8)


def device_ms(fn, iters):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(iters):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) / iters


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=1024)
  ap.add_argument('--iters', type=int, default=50)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'view_ab.txt'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_view needs a HIP device')
  from stackrl_amd import env as envs
  B = args.envs
  env = envs.VecStackEnv(n_parallel=B, seed=11, block=True, episode_length=8)
  env.reset()
  for _ in range(4):
    env.step(env.sample())
  Hm, Om, goal = env.maps()
  H, h = Hm.shape[1], Om.shape[1]
  dm, do = torch.from_numpy(Hm).cuda(), torch.from_numpy(Om).cuda()
  ii = torch.arange(H, device='cuda')
  gl = torch.from_numpy(goal).cuda()
  rows = (ii[None] >= gl[:, :1]) & (ii[None] < gl[:, :1] + gl[:, 2:3])
  cols = (ii[None] >= gl[:, 1:2]) & (ii[None] < gl[:, 1:2] + gl[:, 3:4])
  mask = rows[:, :, None] & cols[:, None, :]
  lines = ['render(rgb_array) of {} envs, {} x {} / {} x {} maps, mid-episode (4 of 8 rocks placed); {}'.format(
    B, H, H, h, h, torch.cuda.get_device_name(0))]
  for dtype in (None, 'uint8'):
    dt = torch.float64 if dtype is None else torch.uint8
    out = (torch.empty((B, H, H, 3), dtype=dt, device='cuda'), torch.empty((B, h, h, 3), dtype=dt, device='cuda'))
    nbytes = out[0].numel() * out[0].element_size() + out[1].numel() * out[1].element_size()
    ms_kernel = device_ms(lambda: env.render(dtype=dtype, out=out), args.iters)
    ms_torch = device_ms(lambda: (torch_rgb(dm, mask, dtype), torch_rgb(do, None, dtype)), args.iters)
    t0 = time.perf_counter()
    reps = 2
    for _ in range(reps):
      ref = vc.batch_reference(env.maps(), vc.rgb_reference if dtype is None else vc.uint8_reference)
    ms_numpy = (time.perf_counter() - t0) / reps * 1e3
    tt = (torch_rgb(dm, mask, dtype), torch_rgb(do, None, dtype))
    same_numpy = all(vc.bits_equal(o.cpu().numpy(), r) for o, r in zip(out, ref))
    same_torch = all(torch.equal(o, t) for o, t in zip(out, tt))
    tbs = nbytes / (ms_kernel * 1e-3) / 1e12
    lines += [
      '{}: {:.1f} MB of images per call'.format(dtype or 'float64', nbytes / 1e6),
      '  kernel (srl_k_view{})   {:9.3f} ms   {:.2f} TB/s stored = {:.0f} % of the {} TB/s an MI355X sustains'.format(
        '' if dtype is None else '_u8', ms_kernel, tbs, 100 * tbs / SUSTAINED_TBS, SUSTAINED_TBS),
      '  torch composition       {:9.3f} ms   {:.1f} x the kernel   bit-equal to the kernel: {}'.format(ms_torch, ms_torch / ms_kernel, same_torch),
      '  maps() + numpy          {:9.3f} ms   {:.0f} x the kernel   bit-equal to the kernel: {}'.format(ms_numpy, ms_numpy / ms_kernel, same_numpy),
    ]
  env.close()
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
