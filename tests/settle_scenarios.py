"""Settle scenarios shared by the settle-variant parity tests (GPU) and the check that they stay hard (CPU, oracle).

Piles: every rock of an episode is dropped near the centre of the map (a few pixels of jitter on the action grid), so that
the rocks land on one another — deep contact graphs, many manifold slots and colours — where random actions mostly put them
side by side on the ground.

Slot-cap arrangements: L cuboids laid out (through `set_body_state`) so that their broadphase boxes overlap in exactly a
chosen number of pairs.  A box is the rock's world AABB grown by collision_margin + 0.01 x radius on every side
(oracle/srl_oracle.c derive_bodies); cuboids with the identity orientation on a grid whose pitch is a fixed fraction of
the grown box make the count a property of the grid: two rocks overlap iff they are at most OVERLAP_STEPS grid steps apart
along every axis, with a margin of a tenth of a box on either side of the threshold (no float32 rounding near it)."""
import numpy as np

CUBOIDS = (64, 65, 66)       # `0_0`, `0_1`, `0_2` of tests/golden/ref_rocks.npz: one shape, three masses
PITCH = 0.45                 # grid pitch as a fraction of the grown box along each axis
OVERLAP_STEPS = 2            # 2 x 0.45 = 0.9 of a box apart: overlap; 3 x 0.45 = 1.35: apart
SCRIPT_SEED = 3              # the pile scripts of the parity tests (and of their hardness check)
ENV_SEED = 7


def pile_script(pool_size, n, L, seed=SCRIPT_SEED):
  """Scripted mesh ids (distinct per env) and goal rectangles."""
  rng = np.random.RandomState(seed)
  ids = np.stack([rng.choice(pool_size, size=L, replace=False) for _ in range(n)]).astype(np.int32)
  rect = np.stack([[rng.randint(8, 40), rng.randint(8, 40), 64, 64] for _ in range(n)]).astype(np.int32)
  return ids, rect, rng


def pile_actions(rng, n, aw):
  """One call's actions: the object window centred on the map, +-3 pixels on the 97 x 97 grid, +-2 on 49 x 49."""
  c, r = aw // 2, (3 if aw > 60 else 2)
  u = c + rng.randint(-r, r + 1, size=n)
  v = c + rng.randint(-r, r + 1, size=n)
  return (u * aw + v).astype(np.int64)


def overlap_pairs(sites):
  """Pairs of grid sites at most OVERLAP_STEPS apart along every axis."""
  s = np.asarray(sites)
  d = np.abs(s[:, None, :] - s[None, :, :]).max(-1)
  return int(np.triu(d <= OVERLAP_STEPS, 1).sum())


def grid_sites(L, pairs, seed=0, extent=(8, 6, 6)):
  """L distinct sites of an extent[0] x extent[1] x extent[2] grid with exactly `pairs` overlapping pairs (a local search
  from a compact block: move one site at a time, keep the move unless it takes the count further from the target)."""
  rng = np.random.RandomState(seed)
  free = [(x, y, z) for z in range(extent[2]) for y in range(extent[1]) for x in range(extent[0])]
  sites = free[:L]
  cur = abs(overlap_pairs(sites) - pairs)
  for _ in range(20000):
    if cur == 0:
      return sorted(sites, key=lambda p: (p[2], p[1], p[0]))
    k = rng.randint(L)
    cand = free[rng.randint(len(free))]
    if cand in sites:
      continue
    trial = sites[:k] + [cand] + sites[k + 1:]
    t = abs(overlap_pairs(trial) - pairs)
    if t <= cur:
      sites, cur = trial, t
  raise AssertionError('no arrangement of {} sites with {} overlapping pairs'.format(L, pairs))


def cuboid_box(pool, cfg):
  """Half extents of a script cuboid and of its grown broadphase box."""
  m = CUBOIDS[0]
  v = pool.verts[pool.vert_off[m]:pool.vert_off[m + 1]].astype(np.float64)
  half = np.abs(v).max(0)
  grow = cfg.collision_margin + 0.01 * np.linalg.norm(v, axis=1).max()
  return half, half + grow


def grid_poses(pool, cfg, sites, x0=(0.0, 0.0)):
  """Poses (the layout of `state()[0]`, rows [x, y, z, qx, qy, qz, qw, -]) of cuboids at grid sites: identity orientation,
  the lowest layer clear of the ground."""
  half, box = cuboid_box(pool, cfg)
  pitch = PITCH * 2.0 * box
  p = np.zeros((len(sites), 8), np.float32)
  for b, s in enumerate(sites):
    p[b, 0] = x0[0] + pitch[0] * s[0]
    p[b, 1] = x0[1] + pitch[1] * s[1]
    p[b, 2] = half[2] + 0.002 + pitch[2] * s[2]
    p[b, 6] = 1.0
  return p


def box_overlap_pairs(pool, cfg, poses):
  """Overlapping grown boxes of axis-aligned script cuboids at `poses`, with the smallest distance of any pair's
  separation (relative to the box) from the threshold: a check of the grid construction in float64."""
  _, box = cuboid_box(pool, cfg)
  x = poses[:, :3].astype(np.float64)
  rel = np.abs(x[:, None, :] - x[None, :, :]) / (2.0 * box)
  iu = np.triu_indices(len(x), 1)
  worst = rel.max(-1)[iu]
  return int((worst <= 1.0).sum()), float(np.abs(rel[iu] - 1.0).min())
