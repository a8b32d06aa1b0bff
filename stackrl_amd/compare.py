"""Comparing policies: the reference's `test` command (`stackrl/test.py`) on the vectorised env.

`run` (test.py:150-353) lets each of P policies drive the env for `num_steps` steps while every policy evaluates every
observation; `analyse` (:412-721) turns what was recorded into return statistics, the mean distance between the policies'
actions, the correlation of their value functions and the overlap of the actions they value above a map's mean and above
its mean + std; `write` (:46-148) keeps `results.csv`; `test` (:723-919) is the command.

The reference keeps every value map — float32 [P, P * num_steps, A], 37.6 KB per policy, env and step at A = 9,409 — and
reduces the array at the end.  Here each vectorised step is reduced where its maps lie to the fixed record of
include/stackrl_compare.h (`MapStatistics`: the kernel of csrc/compare.hip in libstackrl_compare.so on a HIP device, the same
definition in torch on the CPU; `compare_reference` restates it in numpy float64), and the P x P matrices come from the
record.  The value maps themselves are kept only with `keep_values=True`; the histograms of raw values, which need them, are
drawn only then."""
import ctypes
import os

import numpy as np
import torch

from stackrl_amd import _bind

MAX_POLICIES = 8
HOLD = -2          # SRL_ACTION_HOLD (include/srl_types.h): the env sits a call out

_VP, _I32, _INT = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int
# export -> (restype, argtypes, error accessor or None): every declaration of include/stackrl_compare.h (pointers as void*);
# tests/test_abi.py holds the table to the header and the library.  The launching export returns int and takes the
# stream last.
_SIGS = {
  'srl_compare_record_doubles': (_I32, [_I32], None),
  'srl_compare_step': (_INT, [_I32] + [_VP] * 8 + [_I32] * 4 + [_VP] * 5, 'srl_compare_last_error'),
  'srl_compare_last_error': (ctypes.c_char_p, [], None),
  'srl_compare_build_info': (ctypes.c_char_p, [], None),
}


load, call = _bind.binding('compare', _SIGS)


# ------------------------------------------------------------------------------------------------ the record
def _check_P(P):
  P = int(P)
  if not 1 <= P <= MAX_POLICIES:
    raise ValueError('the number of policies must be in 1..{}, got {}'.format(MAX_POLICIES, P))
  return P


def record_doubles(P):
  """R(P) of include/stackrl_compare.h."""
  P = _check_P(P)
  return 1 + P + 5 * (P * (P + 1) // 2)


def pair_index(P):
  """int array [NP, 2]: the pairs i <= j in the record's order."""
  return np.array([(i, j) for i in range(P) for j in range(i, P)], dtype=np.int64).reshape(-1, 2)


def unpack(record, P):
  """A record as a dict: `samples` (steps * B), `s` [P], and the symmetric P x P matrices `S`, `I1`, `U1`, `I2`, `U2`."""
  P = _check_P(P)
  record = np.asarray(record, dtype=np.float64)
  if record.shape != (record_doubles(P),):
    raise ValueError('a record of {} policies has {} numbers, got {}'.format(P, record_doubles(P), record.shape))
  pi = pair_index(P)
  NP = len(pi)
  out = {'samples': record[0], 's': record[1:1 + P].copy()}
  for n, key in enumerate(('S', 'I1', 'U1', 'I2', 'U2')):
    m = np.zeros((P, P))
    seg = record[1 + P + n * NP:1 + P + (n + 1) * NP]
    m[pi[:, 0], pi[:, 1]] = seg
    m[pi[:, 1], pi[:, 0]] = seg
    out[key] = m
  return out


def matrices(record, P, A):
  """{'corrcoef', 'overlap_mean', 'overlap_std'} of a record (test.py:603, :619-656), P x P float64."""
  r = unpack(record, P)
  with np.errstate(divide='ignore', invalid='ignore'):
    n = r['samples'] * float(A)
    m = r['s'] / n
    cov = r['S'] / n - np.outer(m, m)
    d = np.diag(cov)
    den = np.sqrt(np.outer(d, d))
    c = np.clip(cov / den, -1.0, 1.0)             # np.corrcoef does; NaN stays NaN
    c[den == 0] = np.nan                          # a constant map: np.corrcoef's 0 / 0, whatever rounding left in cov
    return {'corrcoef': c, 'overlap_mean': r['I1'] / r['U1'], 'overlap_std': r['I2'] / r['U2']}


def _as_f32_numpy(v):
  if isinstance(v, torch.Tensor):
    v = v.detach().cpu().numpy()
  return np.asarray(v).astype(np.float32)


def compare_reference(values):
  """The definition of include/stackrl_compare.h in numpy float64 on the CPU.

  values: P maps [N, A] (a sequence of arrays or tensors of any float type, or one array [P, N, A]); N counts envs and steps,
  in any order.  Returns (record float64 [R(P)], amax float32 [P, N])."""
  x32 = np.stack([_as_f32_numpy(v) for v in values])
  if x32.ndim != 3 or x32.shape[2] < 1:
    raise ValueError('compare_reference needs P maps [N, A], got {}'.format(x32.shape))
  P = _check_P(x32.shape[0])
  with np.errstate(all='ignore'):
    amax = x32.max(axis=-1)
    x = x32.astype(np.float64)
    mu = x.mean(axis=-1, keepdims=True)
    sigma = np.sqrt(((x - mu) ** 2).mean(axis=-1, keepdims=True))
    f1 = x > mu
    f2 = x > mu + sigma
    pi = pair_index(P)
    rec = [float(x.shape[1])] + [x[j].sum() for j in range(P)]
    rec += [(x[i] * x[j]).sum() for i, j in pi]
    for f in (f1, f2):
      rec += [float(np.count_nonzero(f[i] & f[j])) for i, j in pi]
      rec += [float(np.count_nonzero(f[i] | f[j])) for i, j in pi]
  return np.array(rec, dtype=np.float64), amax


def _chosen_rows(values, actions, A):
  """[B, G * A] or [B, G, A] maps and actions [B] -> the map of each env's chosen row, [B, A] (test.py:274-277)."""
  B = values.shape[0]
  v = values.reshape(B, -1, A)
  row = (actions.to(torch.int64) // A).clamp(0, v.shape[1] - 1)
  return v[torch.arange(B, device=v.device), row]


class MapStatistics(object):
  """The running record of include/stackrl_compare.h for P policies and A actions.

  `step(values, actions=None)`: values is a sequence of P tensors, each one vectorised step's maps [B, A], float32 or float64
  (another float type is converted to float32); with the grouped observation of Stack-v2 the maps are [B, G * A] or [B, G, A]
  and `actions` holds each policy's actions, a sequence of P tensors [B] = row * A + pixel: the map of the chosen row is used.
  Returns amax float32 [P, B].  On a HIP device the kernel of csrc/compare.hip runs and nothing is synchronised; on the CPU
  the same definition in torch.  `result()` returns the record as a numpy array."""

  def __init__(self, P, A, device=None):
    self.P, self.A = _check_P(P), int(A)
    if self.A < 1:
      raise ValueError('A must be positive')
    self.device = torch.device(device if device is not None else 'cpu')
    if self.device.type == 'cuda' and self.device.index is None:
      self.device = torch.device('cuda', torch.cuda.current_device())
    self.R = record_doubles(self.P)
    self.record = torch.zeros(self.R, dtype=torch.float64, device=self.device)
    self._partial = None

  def reset(self):
    self.record.zero_()

  def result(self):
    return self.record.detach().cpu().numpy().copy()

  def _prepare(self, values, actions):
    if len(values) != self.P:
      raise ValueError('{} policies, got {} maps'.format(self.P, len(values)))
    B = values[0].shape[0]
    out = []
    for v in values:
      if v.device != self.device:
        raise ValueError('map on {}, the statistics on {}'.format(v.device, self.device))
      if v.shape[0] != B or v.numel() != values[0].numel() or v.numel() % (B * self.A):
        raise ValueError('maps must be [B, A] or, with actions, [B, G * A]: got {} for A = {}'.format(tuple(v.shape), self.A))
      if v.dtype not in (torch.float32, torch.float64):
        v = v.float()
      out.append(v.contiguous())
    G = out[0].numel() // (B * self.A)
    if G > 1 and actions is None:
      raise ValueError('maps of {} rows per env need the actions that choose the row'.format(G))
    if actions is not None:
      if len(actions) != self.P or any(tuple(a.shape) != (B,) for a in actions):
        raise ValueError('actions must be {} tensors [{}]'.format(self.P, B))
      actions = torch.stack([a.to(device=self.device, dtype=torch.int64) for a in actions]).contiguous()
    return out, actions, B, G

  def step(self, values, actions=None):
    values, actions, B, G = self._prepare(list(values), actions)
    if self.device.type == 'cuda':
      return self._step_device(values, actions, B, G)
    return self._step_torch(values, actions, B, G)

  def _step_device(self, values, actions, B, G):
    if self._partial is None or self._partial.shape[0] < B:
      self._partial = torch.empty((B, self.R), dtype=torch.float64, device=self.device)
    amax = torch.empty((self.P, B), dtype=torch.float32, device=self.device)
    mask = sum(1 << j for j, v in enumerate(values) if v.dtype == torch.float64)
    maps = values + [None] * (MAX_POLICIES - self.P)
    call('srl_compare_step', amax, self.P, *maps, mask, B, G, self.A, actions, amax, self._partial, self.record)
    return amax

  def _step_torch(self, values, actions, B, G):
    P, A = self.P, self.A
    if actions is not None:
      values = [_chosen_rows(v, actions[j], A) for j, v in enumerate(values)]
    x32 = torch.stack([v.reshape(B, A).float() for v in values])             # [P, B, A]
    x = x32.double()
    s = x.sum(-1)
    mu = (s / A)[..., None]
    sigma = torch.sqrt(((x - mu) ** 2).sum(-1) / A)[..., None]
    f1, f2 = x > mu, x > mu + sigma
    pi = pair_index(P)
    i, j = torch.as_tensor(pi[:, 0]), torch.as_tensor(pi[:, 1])
    rec = [torch.tensor([float(B)], dtype=torch.float64, device=x.device), s.sum(-1), (x[i] * x[j]).sum(-1).sum(-1)]
    for f in (f1, f2):
      rec += [(f[i] & f[j]).sum((-1, -2)).double(), (f[i] | f[j]).sum((-1, -2)).double()]
    self.record += torch.cat(rec)
    return x32.amax(-1)


# ------------------------------------------------------------------------------------------------ run (test.py:150-353)
def _named(policies):
  if not isinstance(policies, dict):
    try:
      policies = {str(k): v for k, v in enumerate(policies)}
    except TypeError:
      policies = {'policy': policies}
  for k, v in policies.items():
    if not callable(v):
      raise TypeError('Invalid type {} for element {} of argument policies. Must be callable.'.format(type(v), k))
  return policies


def _wait(step):
  return step() if callable(step) else step


def run(env, policies, num_steps=1024, seed=11, keep_values=False, verbose=False, visualize=None):
  """`run` (test.py:150-353) on a vectorised env of B envs: each policy in turn drives the env for `num_steps` steps, after
  `env.seed(seed)` and `env.reset()` (:259-267), while every policy evaluates every observation.

  policies: a dict name -> callable, an iterable of callables or one callable; a policy takes the batched observation and
  returns (actions int64 [B], values [B, A]); on the grouped observation of Stack-v2 values [B, G * A] and actions
  row * A + pixel (`Baseline(value=True)`, `DQN.greedy(values=True)` / `FusedOrientationGreedy(value=True)`), of which the
  chosen row's map and pixel = action % A are recorded (:274-277).  Under ordering freedom the policy is also given
  `n_valid=env.num_maps_on_show`.
  env: `seed`, `reset`, `step` and `observation_spec` / `batch_size` of `VecStackEnv`.  After a step that ends episodes, the
  envs that are done are reset by one more call, in which the others hold (`SRL_ACTION_HOLD`); that call is not a step.

  Returns a dict: `keys` [P]; `actions` [P, P * num_steps, B, 2], the pixel as (row, column) of the value map, uint8 or uint16;
  `action_values` float32 [P, P * num_steps, B], each map's maximum; `rewards` float32 and `dones` bool [P, num_steps, B];
  `record`, float64 [R(P)]; `n_actions`; and with `keep_values` `values` float32 [P, P * num_steps, B, A].

  visualize: None, or a callable `visualize(step, policy_index, frames)` called before every env step with the picture the
  reference's `visualize=True` shows (test.py:282-317), drawn on the device (`stackrl_amd.valueview`): frames uint8
  [n, FH, FW, 3], one per env of `visualize.envs` (default: every env), drawn by `visualize.view` (default: `ValueView()`);
  `valueview.Recorder` is the standard one.  Its `close()`, if it has one, is called at the end.  What is returned does not
  depend on it."""
  policies = _named(policies)
  keys = np.array(list(policies.keys()))
  P = _check_P(len(keys))
  num_steps = int(num_steps)
  total = P * num_steps
  spec = env.observation_spec
  vshape = (spec[0].shape[-3] - spec[1].shape[-3] + 1, spec[0].shape[-2] - spec[1].shape[-2] + 1)
  A = int(vshape[0] * vshape[1])
  B = int(env.batch_size)
  stats = dev = view = shown = None
  if visualize is not None:
    from stackrl_amd import valueview
    view = getattr(visualize, 'view', None) or valueview.ValueView()
    shown = getattr(visualize, 'envs', None)
  pixels, amaxes, kept, rewards, dones = [], [], [], [], []
  obs = None
  for i in range(total):
    if i % num_steps == 0:
      index = i // num_steps
      if verbose:
        print(str(keys[index]).capitalize())
      env.seed(seed)
      obs = _wait(env.reset())[0]
      if stats is None:
        dev = obs[0].device
        stats = MapStatistics(P, A, dev)
    grouped = obs[1].dim() == 5
    kw = {}
    if grouped and getattr(env, 'num_maps_on_show', obs[1].shape[1]) != obs[1].shape[1]:
      kw['n_valid'] = env.num_maps_on_show
    acts, vals = [], []
    for k in keys:
      a, v = policies[k](obs, **kw)
      acts.append(torch.as_tensor(a, device=dev).to(torch.int64).reshape(B))
      vals.append(torch.as_tensor(v, device=dev).reshape(B, -1))
    amaxes.append(stats.step(vals, acts if grouped else None))
    pixels.append(torch.stack(acts) % A)
    if keep_values:
      kept.append(torch.stack([_chosen_rows(v, a, A).float() for v, a in zip(vals, acts)]))
    if visualize is not None:
      visualize(i % num_steps, index, view.frames(*env.render('rgb_array', dtype='uint8'), vals, acts, index, shown))
    obs, r, d = _wait(env.step(acts[index]))
    if r.dim() != 1:
      raise ValueError('run needs one reward per env, got {}'.format(tuple(r.shape)))
    rewards.append(r.float())
    dones.append(d.bool())
    if bool(d.any()):                    # the reset call: not a step
      hold = torch.where(d.bool(), torch.zeros_like(acts[index]), torch.full_like(acts[index], HOLD))
      obs = _wait(env.step(hold))[0]
  if visualize is not None and callable(getattr(visualize, 'close', None)):
    visualize.close()
  pix = torch.stack(pixels, 1).cpu().numpy()                                  # [P, T, B]
  adt = np.uint8 if max(vshape) < 2 ** 8 else np.uint16
  data = {
    'keys': keys,
    'actions': np.stack(np.unravel_index(pix, vshape), axis=-1).astype(adt),
    'action_values': torch.stack(amaxes, 1).cpu().numpy(),
    'rewards': torch.stack(rewards).reshape(P, num_steps, B).cpu().numpy(),
    'dones': torch.stack(dones).reshape(P, num_steps, B).cpu().numpy(),
    'record': stats.result(),
    'n_actions': A,
  }
  if keep_values:
    data['values'] = torch.stack(kept, 1).cpu().numpy()                       # [P, T, B, A]
  return data


def episode_bounds(dones, b):
  """The reference's `episode_bounds` of env b (test.py:266, :332-342): the steps at which an episode starts, counted over all
  policies, and the total; a trailing partial episode is closed by the next policy's start."""
  P, N = dones.shape[:2]
  bounds = {P * N}
  for p in range(P):
    bounds.add(p * N)
    bounds.update(p * N + int(t) + 1 for t in np.nonzero(dones[p, :, b])[0])
  return np.array(sorted(bounds), dtype=np.uint16 if P * N < 2 ** 16 else np.uint32)


def to_reference(data, b):
  """The dict the reference's `run` returns (test.py:347-353) for env b of a batched run: `keys`, `actions` [P, T, 2],
  `rewards` [P, num_steps], `episode_bounds`, and `values` [P, T, A] if the run kept them."""
  out = {'keys': data['keys'], 'actions': data['actions'][:, :, b], 'rewards': data['rewards'][:, :, b],
         'episode_bounds': episode_bounds(data['dones'], b)}
  if 'values' in data:
    out['values'] = data['values'][:, :, b]
  return out


# ------------------------------------------------------------------------------------------------ analyse (test.py:412-721)
def episode_returns(data):
  """Per policy the float32 returns of its episodes, env after env; a trailing partial episode counts (test.py:335-342,
  :441-448)."""
  rewards, dones = data['rewards'], data['dones']
  P, N, B = rewards.shape
  out = []
  for p in range(P):
    rets = []
    for b in range(B):
      start = 0
      for end in list(np.nonzero(dones[p, :, b])[0] + 1) + [N]:
        if end > start:
          rets.append(rewards[p, start:end, b].sum())
          start = end
    out.append(np.array(rets, dtype=np.float32))
  return out


def _heatmap(plt, matrix, keys, label, path, show):
  fig, ax = plt.subplots()
  im = ax.imshow(matrix)
  fig.colorbar(im, ax=ax).ax.set_ylabel(label, rotation=-90, va='bottom')
  ax.set_xticks(range(len(keys)))
  ax.set_yticks(range(len(keys)))
  ax.set_xticklabels(keys)
  ax.set_yticklabels(keys)
  for i in range(matrix.shape[0]):
    for j in range(matrix.shape[1]):
      ax.text(j, i, '{:.2f}'.format(matrix[i, j]), ha='center', va='center', color='w')
  _finish(plt, path, show)


def _finish(plt, path, show):
  if path:
    plt.savefig(path + '.pdf')
    plt.savefig(path + '.png')
  if show:
    plt.show()
  else:
    plt.close()


def _errorbars(plt, keys, per_policy, ylabel, path, show):
  mean = np.array([x.mean() for x in per_policy])
  lo, hi = np.array([x.min() for x in per_policy]), np.array([x.max() for x in per_policy])
  plt.errorbar(keys, mean, yerr=(mean - lo, hi - mean), fmt='none', ecolor='b', elinewidth=8, alpha=0.25, label='Range')
  plt.errorbar(keys, mean, yerr=np.array([x.std() for x in per_policy]), fmt='bo', capsize=4, label='Mean +/- std dev')
  plt.xlabel('Policy')
  plt.ylabel(ylabel)
  plt.legend(loc='best')
  _finish(plt, path, show)


def analyse(data, show=False, save=None, dirname='.'):
  """`analyse` (test.py:412-721) of what `run` returned.  Returns the reference's keys — `keys`, `return`, `return_std`,
  `action_value`, `action_value_std`, over the episodes and steps of all envs — and the P x P matrices the reference only
  draws: `distance` (the mean distance between the policies' actions, pixels), `corrcoef`, `overlap_mean`, `overlap_std`.

  Plots are drawn only with `show` or `save` (the files go to `dirname`): the return and reward error bars and the four heat
  maps; the histogram of all values of a policy only if the run kept them (`keep_values=True`).  The reference's other
  histograms and its per-step plots are not reproduced."""
  keys = data['keys']
  P = len(keys)
  returns = episode_returns(data)
  av = data['action_values'].reshape(P, -1)
  out = {
    'keys': keys,
    'return': np.array([r.mean() for r in returns], dtype=np.float32),
    'return_std': np.array([r.std() for r in returns], dtype=np.float32),
    'action_value': av.mean(axis=-1),
    'action_value_std': av.std(axis=-1),
  }
  actions = data['actions'].astype(np.int32).reshape(P, -1, 2)
  out['distance'] = np.linalg.norm(actions[None] - actions[:, None], axis=-1).mean(axis=-1)
  out.update(matrices(data['record'], P, data['n_actions']))
  if show or save:
    try:
      import matplotlib.pyplot as plt
    except ImportError:
      raise ImportError('matplotlib must be installed to run analyse with show=True or save=True.')
    if save and not os.path.isdir(dirname):
      os.makedirs(dirname)

    def path(name):
      return os.path.join(dirname, name) if save else None
    _errorbars(plt, keys, returns, 'Return', path('returns'), show)
    _errorbars(plt, keys, list(data['rewards'].reshape(P, -1)), 'Reward', path('rewards'), show)
    if P > 1:
      for name, label in (('distance', 'Mean distance (pixels)'), ('corrcoef', 'Correlation coefficients'),
                          ('overlap_mean', 'Overlap of values above mean'),
                          ('overlap_std', 'Overlap of values one std dev above mean')):
        fname = {'corrcoef': 'correlation', 'overlap_mean': 'overlap_mean', 'overlap_std': 'overlap_std'}.get(name, name)
        _heatmap(plt, out[name], keys, label, path(fname + '_heatmap'), show)
    if 'values' in data:
      for i in range(P):
        plt.hist(data['values'][i].ravel(), bins='auto')
        plt.xlabel('Values (estimated by {})'.format(keys[i]))
        plt.ylabel('Frequency')
        _finish(plt, path('value_hist_{}'.format(keys[i])), show)
  return out


# ------------------------------------------------------------------------------------------------ write (test.py:46-148)
def _column_name(k):
  return ''.join(w[:1].upper() + w[1:] for w in k.split('_'))


def write(fname, force=False, **kwargs):
  """`write` (test.py:46-148): the columns in `kwargs` (scalars are repeated) go to the csv file `fname`, named in CamelCase
  ('action_value' -> 'ActionValue').  A file with the same set of columns is appended to; if there is a column `keys`, the
  lines of the file whose key comes again are replaced, unless there is a column `priority` and the line's is higher than
  the new one's: then the line stays and the new one is dropped.  Other columns: ValueError, or with `force` a new file."""
  n = next((len(v) for v in kwargs.values() if not np.isscalar(v)), None)
  cols = {_column_name(k): (np.array([v] * n) if np.isscalar(v) else np.array(v)) for k, v in kwargs.items()}
  if os.path.isfile(fname):
    with open(fname) as f:
      lines = f.readlines()
    header = lines[0][:-1].split(',')
    if set(header) == set(cols):
      kept, dropped, replaced = [lines[0]], set(), False
      if 'Keys' in header:
        ik = header.index('Keys')
        ip = header.index('Priority') if 'Priority' in header else None
        for line in lines[1:]:
          fields = line[:-1].split(',')
          hit = np.nonzero(cols['Keys'] == fields[ik])[0]
          if len(hit) == 0:
            kept.append(line)
          elif ip is not None and float(fields[ip]) > cols['Priority'][hit[0]]:
            kept.append(line)
            dropped.add(int(hit[0]))
          else:
            replaced = True
      if replaced:
        with open(fname, 'w') as f:
          f.writelines(kept)
      with open(fname, 'a') as f:
        for i, row in enumerate(zip(*[cols[h] for h in header])):
          if i not in dropped:
            f.write(','.join(str(v) for v in row) + '\n')
      return
    if not force:
      raise ValueError("kwargs don't match the existing file's header.")
  if os.path.dirname(fname) and not os.path.isdir(os.path.dirname(fname)):
    os.makedirs(os.path.dirname(fname))
  with open(fname, 'w') as f:
    f.write(','.join(cols.keys()) + '\n')
    for row in zip(*cols.values()):
      f.write(','.join(str(v) for v in row) + '\n')


# ------------------------------------------------------------------------------------------------ test (test.py:723-919)
def test(policies, num_steps=1000, seed=11, save=None, verbose=True, show=False, keep_values=False, plots=None, with_env=None,
         visualize=None, **env_kwargs):
  """The command (test.py:723-919, without the curriculum form): make the env from `env_kwargs` (`stackrl_amd.env.make`), `run`,
  `analyse`, update `results.csv` in the env's directory — lines of a run with more steps are kept (`priority=num_steps`) — and
  print the returns.  `save`: the base directory (a string), True for './data/test', None or False for no files.  `plots`
  (default: as `save`) saves the plots with the files, into `<base>/<env path>/<seed>-<num_steps>/`.  `with_env(env, policies)`
  may return the policies to run once the env exists (policies that need it: `lookahead.LookaheadPolicy`).  `visualize`: as in
  `run`.  Returns the analysis."""
  from stackrl_amd import env as envs
  env = envs.make(**env_kwargs)
  try:
    if with_env is not None:
      policies = with_env(env, policies)
    data = run(env, policies, num_steps=num_steps, seed=seed, keep_values=keep_values, verbose=verbose, visualize=visualize)
  finally:
    env.close()
  base = os.path.join(save if isinstance(save, str) else os.path.join('data', 'test'),
                      envs.env_path(**{k: v for k, v in env_kwargs.items() if k not in ('n_parallel', 'block', 'pool', 'device')}))
  dirname = os.path.join(base, '{}-{}'.format(seed, num_steps))
  result = analyse(data, show=show, save=bool(save) if plots is None else bool(plots and save), dirname=dirname)
  if save and isinstance(policies, dict):              # as in the reference: only named policies leave files
    if not os.path.isdir(dirname):
      os.makedirs(dirname)
    np.savez_compressed(os.path.join(dirname, 'data'), **data)
    write(os.path.join(base, 'results.csv'), priority=num_steps,
          **{k: result[k] for k in ('keys', 'return', 'return_std', 'action_value', 'action_value_std')})
  if verbose:
    print('Average returns (+/- std dev):')
    for n, r, rd in zip(result['keys'], result['return'], result['return_std']):
      print('  {}: {} (+/-{})'.format(n, r, rd))
  return result
