"""The definition of include/stackrl_candidates.h restated in numpy (`reference`): a plain greedy loop over the sorted order.
Also the values, the actions and the list of cases the GPU test runs (tests/test_candidates_gpu.py), which the CPU tests hold
to the properties of the definition (tests/test_candidates_cases.py).  Nothing here imports the library."""
import collections

import numpy as np

MAX_K = 32
THREADS = 1024        # SRL_CANDIDATES_THREADS: an env's entries are dealt to this many threads


def order(v):
  """The indices of v (one env's considered entries, flat) in the order of the definition: NaNs first, then by value
  descending (-0 == +0, -inf last), ties and NaNs by index."""
  nan = np.isnan(v)
  return np.lexsort((-np.where(nan, 0, v), ~nan))          # stable; the last key is the primary one


def reference(values, action, k, radius, n_valid, OH):
  """(cand int64 [B, k], count int32 [B]).  values [B, G * A] float32 or float64 (compared in its own type), action int [B] or None."""
  values = np.asarray(values)
  B = values.shape[0]
  A = OH * OH
  G = values.reshape(B, -1).shape[1] // A
  N = n_valid * A
  assert 1 <= n_valid <= G and 1 <= k <= MAX_K and radius >= 0
  cand = np.zeros((B, k), np.int64)
  count = np.zeros(B, np.int32)
  for b in range(B):
    ranked = order(values.reshape(B, -1)[b, :N])
    struck = np.zeros((G, OH, OH), bool)

    def choose(i):
      g, y, x = i // A, (i % A) // OH, i % OH
      struck[g, max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] = True
      return i
    chosen = [choose(int(np.clip(action[b], 0, G * A - 1)) if action is not None else int(ranked[0]))]
    while len(chosen) < k:
      left = ranked[~struck.reshape(-1)[ranked]]             # the order, without what the candidates so far suppress
      if left.size == 0:
        break
      chosen.append(choose(int(left[0])))
    count[b] = len(chosen)
    cand[b] = chosen + [chosen[0]] * (k - len(chosen))
  return cand, count


# ---- values ------------------------------------------------------------------------------------------------------------

def make_values(kind, B, G, OH, dtype, seed):
  """[B, G * A] of `dtype`.  Every kind is made in float64 first and rounded, so float64 maps hold values float32 would tie."""
  rng = np.random.RandomState(seed)
  A = OH * OH
  if kind == 'random':
    v = rng.standard_normal((B, G, OH, OH))
  elif kind == 'smooth':                # what a policy's map looks like: the best entries are each other's neighbours
    y, x = np.mgrid[:OH, :OH] / max(OH - 1, 1)
    c = rng.rand(B, G, 2, 1, 1)
    v = -((y - c[:, :, 0]) ** 2 + (x - c[:, :, 1]) ** 2) + 1e-3 * rng.standard_normal((B, G, OH, OH))
  elif kind == 'constant':
    v = np.full((B, G, OH, OH), 0.25)
  elif kind == 'quantised':             # four levels: ties everywhere
    v = rng.randint(0, 4, (B, G, OH, OH)) / 4.0
  elif kind == 'edge':                  # the best entries on the last row and the last column
    v = rng.rand(B, G, OH, OH)
    v[:, :, -1, :] += 2
    v[:, :, :, -1] += 2
  elif kind == 'neginf':                # runs of -inf: only a few finite entries per map
    v = rng.standard_normal((B, G, OH, OH))
    v.reshape(B, G, A)[:, :, A // 3:] = -np.inf
    v.reshape(B, G, A)[:, :, :max(A // 8, 0)] = -np.inf
  elif kind == 'nan':                   # NaNs of both signs, +-0, +-inf among ordinary values
    v = rng.standard_normal((B, G, OH, OH))
    flat = v.reshape(-1)
    where = rng.permutation(flat.size)
    n = max(flat.size // 16, 1)
    for j, special in enumerate((np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf)):
      flat[where[j * n:(j + 1) * n]] = special
  elif kind == 'close':                 # neighbours in float64 that are one value in float32
    v = 1.0 + rng.randint(0, 64, (B, G, OH, OH)) * 2.0 ** -40
  else:
    raise ValueError(kind)
  return np.ascontiguousarray(v.reshape(B, G * A).astype(dtype))


def make_action(kind, B, G, OH, n_valid, seed):
  """int64 [B] or None."""
  A = OH * OH
  rng = np.random.RandomState(seed + 1000)
  if kind == 'none':
    return None
  if kind == 'random':                                   # inside the considered maps
    return rng.randint(0, n_valid * A, B).astype(np.int64)
  if kind == 'corners':                                  # the four corners in turn, of the last considered map
    corners = np.array([0, OH - 1, A - OH, A - 1])
    return ((n_valid - 1) * A + corners[np.arange(B) % 4]).astype(np.int64)
  if kind == 'beyond':                                   # in a map >= n_valid (the last one)
    assert n_valid < G
    return ((G - 1) * A + rng.randint(0, A, B)).astype(np.int64)
  if kind == 'outside':                                  # out of range on both sides: clamped
    return np.where(np.arange(B) % 2 == 0, -7 - np.arange(B), G * A + 5 + np.arange(B)).astype(np.int64)
  raise ValueError(kind)


# ---- the cases of the GPU test -----------------------------------------------------------------------------------------

Case = collections.namedtuple('Case', 'name B G n_valid OH k radius dtype values action')


def _case(B=3, G=1, n_valid=None, OH=11, k=8, radius=1, dtype='float32', values='smooth', action='random'):
  n_valid = G if n_valid is None else n_valid
  name = 'B{}-G{}v{}-OH{}-k{}-r{}-{}-{}-{}'.format(B, G, n_valid, OH, k, radius, dtype, values, action)
  return Case(name, B, G, n_valid, OH, k, radius, dtype, values, action)


def cases():
  out = []
  # map size x radius x k (crossed): OH 1 (G = 3, k <= 3), 5, 11 (121 entries: no multiple of a wave or the workgroup),
  # 33 (1,089 entries: a second pass of the workgroup), 97 (the product's); the radius >= OH is exhaustion, and so is k = 32
  # on the 25 entries of OH 5
  for OH in (1, 5, 11, 33, 97):
    for radius in (0, 1, 4, OH + 1):
      for k in (1, 2, 8, 32):
        G = 3 if OH == 1 else 1
        if OH == 1 and k > 3:
          continue
        out.append(_case(B=2 if OH == 97 else 3, G=G, OH=OH, k=k, radius=radius, values='smooth' if OH > 1 else 'random'))
  for radius in (0, 1):
    out.append(_case(G=3, OH=1, k=3, radius=radius, values='random'))
  # G x n_valid x action (crossed) at OH 5 and radius 1
  for G, n_valid in ((1, 1), (4, 1), (4, 3), (4, 4)):
    for action in ('none', 'random', 'corners', 'outside') + (('beyond',) if n_valid < G else ()):
      out.append(_case(B=5, G=G, n_valid=n_valid, OH=5, k=8, radius=1, values='random', action=action))
  # one at a time around the base case: batch, dtype, values
  for B in (1, 130):
    out.append(_case(B=B, values='random'))
  for kind in ('random', 'constant', 'quantised', 'edge', 'neginf', 'nan', 'close'):
    for dtype in ('float32', 'float64'):
      for radius in (0, 1):
        out.append(_case(G=2, dtype=dtype, values=kind, radius=radius, action='none' if kind in ('constant', 'nan') else 'random'))
  out.append(_case(OH=33, G=4, n_valid=3, dtype='float64', values='quantised', radius=4, k=32))
  out.append(_case(OH=97, B=2, dtype='float64', values='smooth', radius=4, action='corners'))
  out.append(_case(OH=97, B=2, G=8, n_valid=8, values='smooth', radius=16, k=32, action='none'))
  names = [c.name for c in out]
  assert len(set(names)) == len(names)
  return out


def inputs(case, seed=0):
  """(values, action) of a case, reproducible from its name."""
  seed = seed + sum(ord(ch) * (j + 1) for j, ch in enumerate(case.name)) % 100003
  return (make_values(case.values, case.B, case.G, case.OH, case.dtype, seed),
          make_action(case.action, case.B, case.G, case.OH, case.n_valid, seed))
