#!/usr/bin/env python3
"""Times `ValueView.frames` (csrc/valueview.hip) at the product's shape — H / h = 128 / 32, P = 6 policies — for scale 2 and 4
and n = 1, 16, 256 frames, beside a torch composition of the same definition (include/stackrl_valueview.h) written here, after
checking that the composition gives the same bytes.

  python tools/bench_value_view.py [--out profiles/value_view.txt] [--repeats 50]

Per shape: the median over `--repeats` timed launches (device events around one call each, after warm-up launches), the bytes
the call stores, that as a share of the store roofline (the 6.3 TB/s of HBM bandwidth an MI355X sustains), and the ratio to the
torch composition.  Frames of n = 1 and 16 fit the last-level cache, so their share of the HBM roofline is a figure of launch
overhead more than of stores."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3
H, h, P, G = 128, 32, 6, 1
GAP, BORDER = 8, 3


def torch_frames(rgb0, rgb1, values, actions, index, indexes, scale, mark, lut, layout, first):
  """The definition as torch operations on the device: uint8 [n, FH, FW, 3]."""
  s, OH = scale, H - h + 1
  A = OH * OH
  n = indexes.shape[0]
  idx = indexes.long()
  frames = torch.full((n, layout['FH'], layout['FW'], 3), 255, dtype=torch.uint8, device=rgb0.device)

  def blocks(img):
    return img.repeat_interleave(s, 1).repeat_interleave(s, 2)
  over = rgb0[idx]
  red = torch.tensor([255, 0, 0], dtype=torch.uint8, device=rgb0.device)
  pixels = [(a[idx] % A) for a in actions]
  if mark:
    u, v = pixels[index] // OH, pixels[index] % OH
    r = torch.arange(H, device=rgb0.device)
    dr, dc = r[None, :, None] - u[:, None, None], r[None, None, :] - v[:, None, None]
    inside = (dr >= 0) & (dr < h) & (dc >= 0) & (dc < h)
    edge = inside & ((dr == 0) | (dr == h - 1) | (dc == 0) | (dc == h - 1))
    over = torch.where(edge[..., None], red, over)
  frames[:, GAP:GAP + s * H, GAP:GAP + s * H] = blocks(over)
  frames[:, 2 * GAP + s * H:2 * GAP + s * (H + h), GAP:GAP + s * h] = blocks(rgb1[idx])
  TB = layout['TB']
  for k in range(layout['nv']):
    j = first + k
    x = values[j].reshape(-1, G, A)[idx, (actions[j][idx] // A).clamp(0, G - 1)].float()
    fin = torch.isfinite(x)
    vmin = torch.where(fin, x, torch.full_like(x, float('inf'))).amin(1, keepdim=True)
    vmax = torch.where(fin, x, torch.full_like(x, float('-inf'))).amax(1, keepdim=True)
    t = (x - vmin) / (vmax - vmin) * 256.0
    t = torch.where(vmax == vmin, torch.zeros_like(t), t)
    q = torch.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0).clamp(0, 255).long()
    cells = torch.where((fin & (vmin <= vmax))[..., None], lut[q], torch.full_like(red, 255))
    if mark:
      cells[torch.arange(n, device=x.device), pixels[j]] = red
    r0, c0 = GAP + (k // 3) * (TB + GAP), 2 * GAP + s * H + (k % 3) * (TB + GAP)
    if j == index:
      frames[:, r0:r0 + TB, c0:c0 + TB] = lut[255]
    frames[:, r0 + BORDER:r0 + TB - BORDER, c0 + BORDER:c0 + TB - BORDER] = blocks(cells.reshape(n, OH, OH, 3))
  return frames


def timed(fn, repeats, warmup=10):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b) * 1e3)
  times = np.array(times)
  return float(np.median(times)), float(np.percentile(times, 10)), float(np.percentile(times, 90))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join('profiles', 'value_view.txt'))
  ap.add_argument('--repeats', type=int, default=50)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('bench_value_view needs a HIP device')
  from stackrl_amd import valueview
  dev = torch.device('cuda', 0)
  gen = torch.Generator(device='cpu').manual_seed(5)
  OH = H - h + 1
  A = OH * OH
  B = 256
  rgb0 = torch.randint(0, 256, (B, H, H, 3), generator=gen, dtype=torch.uint8).to(dev)
  rgb1 = torch.randint(0, 256, (B, h, h, 3), generator=gen, dtype=torch.uint8).to(dev)
  values = [(torch.randn(B, G * A, generator=gen) * 10.0 ** (j - 2)).to(dev) for j in range(P)]
  actions = [torch.randint(0, G * A, (B,), generator=gen).to(dev) for _ in range(P)]
  lut = torch.as_tensor(valueview.lut()).to(dev)
  index = 4
  first = valueview.window(P, index)
  lines = ['ValueView.frames against a torch composition of the same definition: H / h = {} / {}, P = {}, B = {}, mark on, '
           'driving policy {}'.format(H, h, P, B, index),
           'device: {}; torch {}; median (10th .. 90th percentile) of {} launches timed one by one with device events, after 10 '
           'warm-up launches; each kernel call is srl_valueview_frames = k_value_range + k_value_frame'.format(
             torch.cuda.get_device_name(0), torch.__version__, args.repeats),
           'share of the store roofline = bytes stored / {} TB/s over the median'.format(HBM_TBS), '']
  slower = []
  for s in (2, 4):
    layout = valueview.layout(H, h, P, s)
    view = valueview.ValueView(scale=s, mark=True)
    for n in (1, 16, 256):
      indexes = torch.arange(n, dtype=torch.int32, device=dev)
      out = torch.empty((n, layout['FH'], layout['FW'], 3), dtype=torch.uint8, device=dev)
      got = view.frames(rgb0, rgb1, values, actions, index=index, indexes=indexes, out=out)
      want = torch_frames(rgb0, rgb1, values, actions, index, indexes, s, True, lut, layout, first)
      if not torch.equal(got, want):
        raise SystemExit('the torch composition and the kernel differ at scale {} n {}: {} bytes'.format(
          s, n, int((got != want).sum())))
      k = timed(lambda: view.frames(rgb0, rgb1, values, actions, index=index, indexes=indexes, out=out), args.repeats)
      t = timed(lambda: torch_frames(rgb0, rgb1, values, actions, index, indexes, s, True, lut, layout, first), args.repeats)
      nbytes = out.numel()
      if n == 16 and k[0] >= t[0]:
        slower.append(s)
      lines.append('scale {} n {:3d}  frame {} x {}  {:11d} bytes stored   kernel {:9.1f} us ({:.1f} .. {:.1f})  {:5.1f} % of the store '
                   'roofline   torch {:9.1f} us ({:.1f} .. {:.1f})   torch / kernel = {:.1f}   bytes equal'.format(
                     s, n, layout['FH'], layout['FW'], nbytes, k[0], k[1], k[2], 100 * nbytes / (HBM_TBS * 1e12) / (k[0] * 1e-6),
                     t[0], t[1], t[2], t[0] / k[0]))
  lines.append('')
  lines.append('the kernel is NOT faster than the torch composition at n = 16 for scale {}'.format(slower) if slower else
               'the kernel is faster than the torch composition at n = 16 for both scales')
  text = '\n'.join(lines) + '\n'
  print(text)
  if os.path.dirname(args.out):
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
