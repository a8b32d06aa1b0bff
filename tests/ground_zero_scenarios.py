"""Scenarios in which the settle solver's rows meet EXACT zeros, shared by test_ground_zero_terms.py (CPU: the oracle alone, that
the scenarios are what they are for) and test_ground_zero_terms_gpu.py (every settle kernel against the oracle).

The kernels leave the products with a ground row's structural zeros out of its chain, share the four distinct words of a
ground point's ca vectors and form a friction row's impulse as a plain product (stackrl_amd/csrc/solver.h, "The rows'
structural zeros"): where the oracle's full expression is an exact zero, the kernels' can be the zero of the other sign.  The
random rocks of the parity suite never get there; axis-aligned cuboids at rest do.  Every env holds L cuboids with the
identity orientation, each flat on the ground on a site of its own, far from the others — all their rows have vrel = 0 on
the first sub-step — and on top of that, per env:

  env 0  FALL      cuboid 0 with v = (0, 0, -0.1), w = 0
  env 1  STACK     cuboid 1 flat on top of cuboid 0, both with v = (0, 0, -0.1): pair rows with zero lateral velocities
  env 2  SLIDE     cuboid 0 with v = (0.05, 0, 0), cuboid 1 with v = (0, -0.05, 0): one lateral component each, the rest zero
  env 3  TARGET0   every cuboid at the height where dist + linear_slop == 0 in float32 (the normal row's target is -0) and
                   with the upward speed gravity cancels exactly (vrel = 0 too: every impulse is a zero, nothing moves)
  env 4  HOVER     every cuboid GAP above contact with that upward speed, cuboid 1 GAP above cuboid 0, cuboid 2 with
                   v.x = 0.05 and cuboid 3 with v.y = -0.05 besides: on the first sub-step every ground and pair point
                   exists, its normal row wants to pull (clamped to 0), its friction rows have the bounds -0, +0 and
                   vrel = 0 or one lateral component — the impulses are zeros of either sign and the zero components
                   of the velocities survive the solve; from the second sub-step on the cuboids land
  env 5  REST      nothing added

In envs 0 - 2 and 5 the cuboids are pressed SINK into the ground's margin: their first sub-step pushes them out (non-zero
normal impulses on velocities whose other components start as zeros).

`place` needs handles with n_envs = N_ENVS, episode_length = L (L >= 4) and the settings CFG: collision_margin and
linear_slop one binade-aligned step from their defaults (0.001 -> 2^-10, 1e-5 -> 2^-17).  A bottom vertex's height is a
multiple of 2^-28 at these sizes, and float32(0.001) - float32(1e-5) is not: with the defaults no pose has
dist + linear_slop == 0."""
import numpy as np

import settle_scenarios as S

N_ENVS = 6
FALL, STACK, SLIDE, TARGET0, HOVER, REST = range(N_ENVS)
SUBSTEPS = 24
CFG = dict(collision_margin=2.0 ** -10, linear_slop=2.0 ** -17)
SINK = 0.0005                # flat "on" the ground / on a cuboid: this far inside the contact margin
GAP = 0.0002                 # hovering: this far outside it (the contact threshold is 0.02 x the radius, about 0.0012)


def f32(x):
  return np.float32(x)


def cuboid_half(pool):
  """Half extents of the script cuboids, checked to be exact: every vertex is (+-hx, +-hy, +-hz) in the body frame."""
  m = S.CUBOIDS[0]
  v = pool.verts[pool.vert_off[m]:pool.vert_off[m + 1]]
  half = np.abs(v).max(0).astype(np.float32)
  assert np.array_equal(np.abs(v).astype(np.float32), np.broadcast_to(half, v.shape)), 'the script cuboid is no centred box'
  return half


def target0_height(cfg, half):
  """The centre height z at which a flat cuboid's bottom vertices have dist + linear_slop == 0 in the kernels' float32
  arithmetic: wz = z - hz, dist = wz - collision_margin, pen = dist + linear_slop."""
  m, slop, hz = f32(cfg.collision_margin), f32(cfg.linear_slop), f32(half[2])
  z = f32(f32(m - slop) + hz)
  for _ in range(256):
    for cand in (z, np.nextafter(z, f32(0.0))):
      if f32(f32(f32(cand - hz) - m) + slop) == 0.0:
        return cand
    z = np.nextafter(z, f32(np.inf))
  raise AssertionError('no float32 height with dist + linear_slop == 0')


def cancel_speed(cfg):
  """vz with vz * lin_damp - gravity * dt == 0 in float32 (the oracle's damping factor: pow in double, rounded to float)."""
  dt, g = f32(cfg.sim_time_step), f32(cfg.gravity)
  damp = f32(np.power(1.0 - float(f32(cfg.linear_damping)), float(dt)))
  want = f32(g * dt)
  vz = f32(want / damp)
  for _ in range(64):
    for cand in (vz, np.nextafter(vz, f32(0.0))):
      if f32(cand * damp) == want:
        return cand
    vz = np.nextafter(vz, f32(np.inf))
  raise AssertionError('no float32 speed that gravity cancels exactly')


def place(handles, pool, cfg, L):
  """Every handle (oracle or GPU, the same shape) with L cuboids placed, then set to the scenarios.  Returns (poses, velocities)."""
  n = cfg.n_envs
  assert n == N_ENVS and L >= 4
  ids = np.tile(np.resize(np.asarray(S.CUBOIDS, np.int32), L), (n, 1))
  rect = np.array([[40, 40, 64, 64]] * n, np.int32)
  aw = cfg.overhead_res - cfg.object_res + 1
  a = np.full(n, (aw // 2) * aw + aw // 2, np.int64)
  for h in handles:
    h.set_script(ids, rect)
    h.reset()
  for _ in range(L):
    for h in handles:
      if hasattr(h, 'step_variant'):
        import torch
        h.step(torch.from_numpy(a).cuda())
      else:
        h.step(a)
  half = cuboid_half(pool)
  _, box = S.cuboid_box(pool, cfg)
  p = np.array(handles[0].state()[0], np.float32)
  v = np.zeros_like(p)
  z0 = f32(f32(half[2]) + f32(cfg.collision_margin - SINK))
  for e in range(n):
    for b in range(L):              # sites three boxes apart on a row-major grid: no broadphase pair between them
      p[e, b, :7] = (6.0 * box[0] * (b % 6), 6.0 * box[1] * (b // 6), z0, 0.0, 0.0, 0.0, 1.0)
      p[e, b, 7] = ids[e, b]
  v[FALL, 0, 2] = -0.1
  p[STACK, 1, :3] = p[STACK, 0, :3]
  p[STACK, 1, 2] = f32(z0 + f32(2.0 * half[2]) + f32(2.0 * cfg.collision_margin - SINK))
  v[STACK, :2, 2] = -0.1
  v[SLIDE, 0, 0] = 0.05
  v[SLIDE, 1, 1] = -0.05
  vz = cancel_speed(cfg)
  p[TARGET0, :L, 2] = target0_height(cfg, half)
  v[TARGET0, :L, 2] = vz
  zh = f32(f32(half[2]) + f32(cfg.collision_margin + GAP))
  p[HOVER, :L, 2] = zh
  p[HOVER, 1, :3] = p[HOVER, 0, :3]
  p[HOVER, 1, 2] = f32(zh + f32(2.0 * half[2]) + f32(2.0 * cfg.collision_margin + GAP))
  v[HOVER, :L, 2] = vz
  v[HOVER, 2, 0] = 0.05
  v[HOVER, 3, 1] = -0.05
  up = p.copy()
  up[:, :, 2] += 1.0
  for h in handles:
    h.set_body_state(up, v)         # one sub-step in the air: the manifolds of the placing steps, and the impulses they
    h.step_simulation(1)            # would warm-start the scenarios with, are gone
    h.set_body_state(p, v)
  return p, v


def run(h, substeps=SUBSTEPS):
  """`substeps` single sub-steps on handle h: per sub-step (poses, velocities, sub-step counts, sweeps, statuses, contacts)."""
  out = []
  for _ in range(substeps):
    h.step_simulation(1)
    poses, _, sub, st = h.state()
    out.append((poses.copy(), h.velocities().copy(), sub.copy(), h.sweeps().copy(), st.copy(),
                tuple(np.copy(c) for c in h.contacts())))
  return out
