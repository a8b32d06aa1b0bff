#!/usr/bin/env python3
"""Look at what a policy builds: run N Stack-v0 envs for one episode with a heuristic baseline, or with the greedy policy of
a Q-network's saved weights, and write the frames `env.render('rgb_array', dtype='uint8')` gives after the reset and after
every placement — what the reference shows with `env.render()` at every step of a visualised run (stackrl/test.py:283).

  python tools/render_episode.py [--envs 4] [--episode-length 8] [--baseline height | --weights FILE] [--show 0,1]
                                 [--out frames] [--seed 11] [--camera [--yaw 45 --pitch -45 --distance D --size 320x240]]

Written under --out, with no plotting library: `env<i>_step<k>.ppm` (binary PPM: the overhead view with the object view in
its top right corner, on a margin of its own) for the envs of --show, and `frames.npy`, uint8 [steps + 1, shown, H, H + h, 3].
With --camera the perspective view of the pile itself (`env.render_camera`: the rocks on the ground, the observable square, the
goal rectangle, shadows — the reference's GUI view unless --yaw / --pitch / --distance say otherwise) is written beside them:
`env<i>_step<k>_camera.ppm` and `camera.npy`, uint8 [steps + 1, shown, height, width, 3]."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def side_by_side(rgb0, rgb1):
  """uint8 [B, H, H, 3] and [B, h, h, 3] -> [B, H, H + h, 3]: the object view right of the overhead view, black below it."""
  B, H, h = rgb0.shape[0], rgb0.shape[1], rgb1.shape[1]
  out = np.zeros((B, H, H + h, 3), np.uint8)
  out[:, :, :H] = rgb0
  out[:, :h, H:] = rgb1
  return out


def write_ppm(path, image):
  """One uint8 [rows, columns, 3] image as a binary PPM (P6)."""
  image = np.ascontiguousarray(image, np.uint8)
  assert image.ndim == 3 and image.shape[2] == 3
  with open(path, 'wb') as f:
    f.write('P6\n{} {}\n255\n'.format(image.shape[1], image.shape[0]).encode())
    f.write(image.tobytes())


def write_frames(dirname, frames, shown, suffix='', stack='frames.npy'):
  """frames: uint8 [steps, len(shown), rows, columns, 3] -> one PPM per env and step + the stack as .npy; returns the paths."""
  os.makedirs(dirname, exist_ok=True)
  paths = []
  for k in range(frames.shape[0]):
    for j, i in enumerate(shown):
      paths.append(os.path.join(dirname, 'env{}_step{}{}.ppm'.format(i, k, suffix)))
      write_ppm(paths[-1], frames[k, j])
  paths.append(os.path.join(dirname, stack))
  np.save(paths[-1], frames)
  return paths


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--envs', type=int, default=4)
  ap.add_argument('--episode-length', type=int, default=8)
  ap.add_argument('--seed', type=int, default=11)
  ap.add_argument('--baseline', default='height', help='a method of stackrl_amd.baselines (random, height, difference, corrcoef, ...)')
  ap.add_argument('--weights', default=None, help='a file written by DQN.save_weights: the greedy policy of that network instead')
  ap.add_argument('--show', default='0', help='comma-separated env indices whose frames are written')
  ap.add_argument('--out', default='frames')
  ap.add_argument('--camera', action='store_true', help='also write the perspective view of the pile (env.render_camera)')
  ap.add_argument('--yaw', type=float, default=45., help='degrees; with --pitch and --distance: stackrl_amd/camera.py')
  ap.add_argument('--pitch', type=float, default=-45.)
  ap.add_argument('--distance', type=float, default=None, help='metres from the middle of the observable square; default: the reference\'s')
  ap.add_argument('--size', default='320x240', help='WIDTHxHEIGHT of the camera frames')
  args = ap.parse_args()
  try:
    cam_w, cam_h = (int(x) for x in args.size.lower().split('x'))
  except ValueError:
    raise SystemExit('--size must be WIDTHxHEIGHT')
  if not torch.cuda.is_available():
    raise SystemExit('render_episode needs a HIP device')
  shown = [int(i) for i in args.show.split(',') if i != '']
  if not shown or min(shown) < 0 or max(shown) >= args.envs:
    raise SystemExit('--show must name envs in 0..{}'.format(args.envs - 1))
  from stackrl_amd import env as envs
  env = envs.make('Stack-v0', n_parallel=args.envs, episode_length=args.episode_length, seed=args.seed, block=True)
  if args.weights:
    from stackrl_amd import nets, qops
    from stackrl_amd.dqn import DQN
    net = nets.DeepQSiamFCN(env.observation_spec, seed=0).cuda()
    net.load_state_dict(torch.load(args.weights, map_location='cuda'))
    agent = DQN(net, collect_batch_size=args.envs, replay_memory_size=2 * args.envs, seed=0, policy_op=qops.FusedPolicy(fast=True),
                xcorr='bf16x3')
    policy = agent.greedy
  else:
    from stackrl_amd.baselines import Baseline
    policy = Baseline(args.baseline, seed=args.seed if args.baseline == 'random' else None)
  idx = torch.as_tensor(shown, device='cuda')
  frames, views, total = [], [], torch.zeros(args.envs, device='cuda')
  camera = None
  if args.camera:
    from stackrl_amd.camera import Camera
    sx = env.config.overhead_res * env.config.pixel_size
    distance = args.distance if args.distance is not None else (2 * sx * sx + env.config.max_z ** 2) ** 0.5      # env.py:275-281
    camera = Camera.look_at((sx / 2, sx / 2, 0.), distance, args.yaw, args.pitch)

  def grab():
    rgb0, rgb1 = env.render('rgb_array', dtype='uint8')
    frames.append(side_by_side(rgb0[idx].cpu().numpy(), rgb1[idx].cpu().numpy()))
    if camera is not None:
      views.append(env.render_camera(cam_w, cam_h, camera=camera)[idx].cpu().numpy())

  obs, _, _ = env.reset()
  grab()
  for _ in range(args.episode_length):
    obs, reward, done = env.step(policy(obs))
    total += reward
    grab()
  assert bool(done.all())
  paths = write_frames(args.out, np.stack(frames), shown)
  if views:
    paths += write_frames(args.out, np.stack(views), shown, suffix='_camera', stack='camera.npy')
  print('policy: {}; returns of the shown envs: {}'.format(args.weights or args.baseline, [round(float(total[i]), 4) for i in shown]))
  print('wrote {} files under {} ({} frames of {} envs, {} x {})'.format(len(paths), args.out, len(frames), len(shown), *frames[0].shape[1:3]))
  env.close()


if __name__ == '__main__':
  main()
