#!/usr/bin/env python3
"""Time `render_camera` (csrc/camera.hip, srl_k_camera) on piles an env has built — 1,024 envs x 8 rocks and 4,096 x 16, at
160 x 120 and 320 x 240, with and without shadows — beside a straightforward torch composition of the same definition on the
same device:

  kernel   `env.render_camera(w, h, out=...)` of the whole batch (rgb + depth + ids): one launch, every launch between its
           own pair of device events after a warm-up, the median over --iters launches
  torch    the definition written with torch operations (planes gathered per body, one [envs, faces, rays] tensor per
           body for the denominators and quotients, max / min over the faces, the shadow rays the same way).  Its temporaries
           are [envs, faces, rays] float32, so it runs on --torch-envs envs at a time; it is timed on that many envs and its
           time per env is what the ratio uses (eager torch at these sizes is linear in the envs)

Reports microseconds per launch, eye rays per second (envs x width x height over the time: shadow rays are not counted), the
ratio, and how many of the ids of the two routes agree.  The clocks are left as they are found and named in the output.

  python tools/bench_camera.py [--iters 20] [--torch-envs 8] [--out profiles/camera_view.txt] [--quick]"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ((1024, 8), (4096, 16))
SIZES = ((160, 120), (320, 240))


def plane_table(pool):
  """float32 [n_mesh, F, 4] unit face planes in the centre-of-mass frame (float64 arithmetic, rounded) and the face counts;
  the faces past a mesh's own are (0, 0, 0, 1): parallel to every ray and never shutting one out."""
  nf = np.diff(pool.tri_off)
  tab = np.zeros((len(pool), int(nf.max()), 4), np.float32)
  tab[:, :, 3] = 1.0
  for m in range(len(pool)):
    v, t, mc = pool.mesh(m)
    a = v.astype(np.float64) - mc[1:4].astype(np.float64)[None]
    n = np.cross(a[t[:, 1]] - a[t[:, 0]], a[t[:, 2]] - a[t[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    tab[m, :len(t), :3], tab[m, :len(t), 3] = n, (n * a[t[:, 0]]).sum(1)
  return torch.from_numpy(tab).cuda(), torch.from_numpy(nf.astype(np.int64)).cuda()


def _clip(num, den, valid):
  t = num / den
  ninf, pinf = torch.tensor(-np.inf, device=t.device), torch.tensor(np.inf, device=t.device)
  tin, fin = torch.where((den < 0) & valid, t, ninf).max(1)
  tout = torch.where((den > 0) & valid, t, pinf).min(1).values
  miss = ((den == 0) & (num < 0) & valid).any(1)
  return tin, fin, tout, miss


def torch_camera(tab, nf, poses, mesh, nb, goal, c, px, res):
  """The definition of include/stackrl_hip.h for envs [B]: poses [B, L, 7], mesh [B, L], nb [B], goal [B, 4] device tensors,
  c the `srl_camera` struct -> rgb uint8 [B, H, W, 3], depth [B, H, W], ids int32 [B, H, W]."""
  dev = poses.device
  B, L = mesh.shape
  W, H = c.width, c.height
  f = lambda a: torch.tensor([a[0], a[1], a[2]], dtype=torch.float32, device=dev)
  eye, fwd, right, up, light = f(c.eye), f(c.fwd), f(c.right), f(c.up), f(c.light)
  s = (2 * torch.arange(W, device=dev) + 1).float() / W - 1
  u = 1 - (2 * torch.arange(H, device=dev) + 1).float() / H
  d = ((fwd[None, None] + s[None, :, None] * right[None, None]) + u[:, None, None] * up[None, None]).reshape(-1, 3)     # [P, 3]
  P = d.shape[0]
  best = torch.full((B, P), np.inf, device=dev)
  bid = torch.full((B, P), -1, dtype=torch.int64, device=dev)
  nrm = torch.zeros((B, P, 3), device=dev)
  world = []
  for b in range(L):
    pl = tab[mesh[:, b].long()]                                               # [B, F, 4]
    x, q = poses[:, b, :3], poses[:, b, 3:7]
    qx, qy, qz, qw = q.unbind(1)
    R = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                     2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                     2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)], 1).view(B, 3, 3)
    nw = pl[:, :, :3] @ R.transpose(1, 2)                                      # [B, F, 3]
    dw = pl[:, :, 3] + (nw * x[:, None]).sum(-1)
    valid = ((torch.arange(pl.shape[1], device=dev)[None] < nf[mesh[:, b].long()][:, None]) & (b < nb)[:, None])[:, :, None]
    world.append((nw, dw, valid, (b < nb)[:, None]))
    den = nw @ d.t()[None]                                                     # [B, F, P]
    num = (dw - nw @ eye)[:, :, None].expand_as(den)
    tin, fin, tout, miss = _clip(num, den, valid)
    take = ~miss & (tin < tout) & (tin > 0) & (tin < best)
    best, bid = torch.where(take, tin, best), torch.where(take, torch.full_like(bid, b), bid)
    nrm = torch.where(take[:, :, None], torch.gather(nw, 1, fin[:, :, None].expand(-1, -1, 3)), nrm)
  tg = torch.where(d[:, 2] < 0, -eye[2] / d[:, 2], torch.full_like(d[:, 2], np.inf))[None].expand(B, -1)
  rock = (bid >= 0) & (best < tg)
  ground = ~rock & (d[:, 2] < 0)[None]
  ids = torch.where(rock, bid, torch.where(ground, torch.full_like(bid, -1), torch.full_like(bid, -2)))
  t = torch.where(rock, best, torch.where(ground, tg, torch.full_like(best, np.inf)))
  up_n = torch.tensor([0., 0., 1.], device=dev)
  nrm = torch.where(rock[:, :, None], nrm, up_n[None, None])
  seen = ids != -2
  p = eye[None, None] + torch.where(seen, t, torch.zeros_like(t))[:, :, None] * d[None]
  lit = torch.ones((B, P), device=dev)
  if c.shadows:
    o = p + 1e-4 * nrm
    blocked = torch.zeros((B, P), dtype=torch.bool, device=dev)
    for nw, dw, valid, exists in world:
      num = dw[:, :, None] - nw @ o.transpose(1, 2)
      den = (nw @ light)[:, :, None].expand_as(num)
      tin, _, tout, miss = _clip(num, den, valid)
      blocked |= exists & ~miss & (tin < tout) & (tout > 0)
    lit = torch.where(blocked & seen, torch.zeros_like(lit), lit)
  sx = float(res) * float(px)
  g = goal.float() * float(px)
  g1 = (goal[:, :2] + goal[:, 2:]).float() * float(px)
  obs = ground & (p[..., 0] >= 0) & (p[..., 0] <= sx) & (p[..., 1] >= 0) & (p[..., 1] <= sx)
  ing = obs & (p[..., 0] >= g[:, None, 0]) & (p[..., 0] <= g1[:, None, 0]) & (p[..., 1] >= g[:, None, 1]) & (p[..., 1] <= g1[:, None, 1])
  albedo = torch.full((B, P, 3), 0.8, device=dev)
  albedo = torch.where(obs[:, :, None], 0.5 * albedo + 0.5, albedo)
  albedo = torch.where(ing[:, :, None], 0.5 * albedo + 0.5 * torch.tensor([0., 1., 0.], device=dev)[None, None], albedo)
  albedo = torch.where(rock[:, :, None], f(c.rock_rgb)[None, None], albedo)
  shade = c.ambient + (c.diffuse * (nrm @ light).clamp(min=0)) * lit
  rgb = torch.where(seen[:, :, None], albedo * shade[:, :, None], f(c.sky_rgb)[None, None])
  rgb8 = (rgb.double() * 255 + 0.5).clamp(0, 255).to(torch.uint8)
  return rgb8.view(B, H, W, 3), t.view(B, H, W), ids.view(B, H, W).int()


def launches_us(fn, iters, warmup=3):
  """Median and spread (min, max) in microseconds of `fn`, each call between its own pair of device events."""
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
  for a, b in ev:
    a.record()
    fn()
    b.record()
  torch.cuda.synchronize()
  us = [a.elapsed_time(b) * 1e3 for a, b in ev]
  return statistics.median(us), min(us), max(us)


def clock_state():
  """The clocks as they are found (nothing is set): what rocm-smi shows, or that it could not be asked."""
  try:
    out = subprocess.run(['rocm-smi', '--showperflevel', '--showclocks', '-d', '0'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                         timeout=20, universal_newlines=True).stdout
    keep = [l.strip() for l in out.splitlines() if 'Performance Level' in l or 'sclk' in l or 'mclk' in l]
    return '; '.join(keep) if keep else 'rocm-smi printed no clock lines'
  except Exception as e:      # noqa: BLE001 (a tool that is missing or hangs must not cost the measurement)
    return 'not read ({})'.format(type(e).__name__)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--torch-envs', type=int, default=8)
  ap.add_argument('--torch-iters', type=int, default=3)
  ap.add_argument('--quick', action='store_true', help='64 envs x 3 rocks and 8 x 4, to rehearse the script')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'camera_view.txt'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_camera needs a HIP device')
  from stackrl_amd import env as envs
  from stackrl_amd.camera import Camera
  lines = ['render_camera (srl_k_camera: rgb + depth + ids) of piles the envs built, reference view; {}'.format(torch.cuda.get_device_name(0)),
           'clocks as found before the first launch, nothing set: {}'.format(clock_state()),
           'kernel: median (min .. max) of {} launches, each between device events, after 3 warm-up launches; torch: the same '
           'definition composed of torch operations, timed on {} envs ({} runs, median) and scaled to the batch'.format(args.iters, args.torch_envs, args.torch_iters)]
  for B, L in (((64, 3), (8, 4)) if args.quick else CONFIGS):
    env = envs.VecStackEnv(n_parallel=B, seed=11, block=True, episode_length=L)
    env.reset()
    for _ in range(L):
      env.step(env.sample())
    poses, nb, _, _ = env.state()
    goal = env.maps()[2]
    assert (nb == L).all()
    tab, nf = plane_table(env.pool)
    T = min(args.torch_envs, B)
    tp = torch.from_numpy(poses[:T, :L, :7].copy()).cuda()
    tm = torch.from_numpy(poses[:T, :L, 7].astype(np.int64)).cuda()
    tn, tgoal = torch.from_numpy(nb[:T].astype(np.int64)).cuda(), torch.from_numpy(goal[:T].astype(np.int64)).cuda()
    lines.append('{} envs x {} rocks'.format(B, L))
    for w, h in SIZES:
      out = [torch.empty((B, h, w, 3), dtype=torch.uint8, device='cuda'), torch.empty((B, h, w), dtype=torch.float32, device='cuda'),
             torch.empty((B, h, w), dtype=torch.int32, device='cuda')]
      for shadows in (False, True):
        cam = Camera.reference(env.config, shadows=shadows)
        c = cam.to_c(w, h)
        med, lo, hi = launches_us(lambda: env.render_camera(w, h, camera=cam, rgb=True, depth=True, ids=True, out=out), args.iters)
        tmed, _, _ = launches_us(lambda: torch_camera(tab, nf, tp, tm, tn, tgoal, c, env.config.pixel_size, env.config.overhead_res),
                                 args.torch_iters, warmup=1)
        ref = torch_camera(tab, nf, tp, tm, tn, tgoal, c, env.config.pixel_size, env.config.overhead_res)
        same = float((ref[2] == out[2][:T]).float().mean())
        close = float(((ref[0].int() - out[0][:T].int()).abs().amax(-1) <= 1).float().mean())
        torch_batch = tmed * B / T
        lines.append('  {:3d} x {:3d} {:10s}  kernel {:10.1f} us ({:.1f} .. {:.1f})  {:8.2f} G eye rays/s   torch {:12.1f} us for the batch '
                     '({:.1f} us on {} envs)  ratio {:7.1f}   ids equal {:.4f}, rgb within a level {:.4f}'.format(
                       w, h, 'shadows' if shadows else 'no shadows', med, lo, hi, B * w * h / med * 1e-3, torch_batch, tmed, T, torch_batch / med, same, close))
        print(lines[-1], flush=True)
    env.close()
  lines.insert(2, 'clocks right after the last launch: {}'.format(clock_state()))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
