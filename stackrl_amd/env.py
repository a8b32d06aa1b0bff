"""Host-side mirror of the reference's batched env interface over the HIP C-ABI.

`VecStackEnv` is what `stackrl.envs.make('Stack-v0', n_parallel=B, seed=s, **kwargs)` returns in
the reference (`stackrl/envs/utils.py:44-141` -> `ParallelEnv`, `:302-576`): same method and property
names (`step/reset/sample/seed/close/__call__`, `batch_size`, `observation_spec`, `action_spec`,
`multiprocessing`), same argument meaning, same tuple layout
`((u8[B,H,W,2], u8[B,h,w,1]), f32[B], bool[B])` (u8: the `dtype` argument's type, uint8 by default), same
non-blocking default (a callable that yields the time step, `utils.py:468-486`), same exception types.  Tensors are torch
(ROCm) instead of tf.

All arithmetic happens in libstackrl_hip.so; torch only owns device memory and streams.
"""
import collections
import ctypes
import os

import numpy as np
import torch

from stackrl_amd import assets as _assets
from stackrl_amd import lib as _lib
from stackrl_amd import config as _config
from stackrl_amd import state as _state
from stackrl_amd.config import StackConfig

TensorSpec = collections.namedtuple('TensorSpec', ['shape', 'dtype'])

# the observation's element type per `dtype` argument (env.py:24, :168-180; StackConfig.dtype)
TORCH_DTYPES = {'uint8': torch.uint8, 'uint16': torch.uint16, 'uint32': torch.uint32, 'uint64': torch.uint64,
                'float16': torch.float16, 'float32': torch.float32, 'float64': torch.float64}


def _check(rc):
  if rc == _config.OK:
    return
  msg = _lib.last_error()
  if rc == _config.EINVAL_ACTION:
    raise AssertionError(msg)             # env.py:238
  if rc == _config.ESIM_DIVERGED:
    raise RuntimeError(msg)               # simulator.py:221-224
  if rc in (_config.EINVAL, _config.ENOMESH):
    raise ValueError(msg)
  raise RuntimeError('HIP error: ' + msg)


def _np_ptr(a):
  return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# the image types of `render` -> srl_render_rgb's dtype codes (include/stackrl_hip.h)
VIEW_DTYPES = {'float64': 0, 'uint8': 1}


def _view_dtype(dtype):
  """(srl_render_rgb code, torch dtype) of `render`'s dtype argument — a name, a torch or a numpy type; None = float64, what
  the reference returns.  Code -1 for a type the export does not write."""
  if dtype is None:
    name = 'float64'
  elif isinstance(dtype, torch.dtype):
    name = str(dtype).split('.')[-1]
  else:
    try:
      name = np.dtype(dtype).name
    except TypeError:
      name = str(dtype)
  return VIEW_DTYPES.get(name, -1), TORCH_DTYPES.get(name)


class VecStackEnv(object):
  """B independent Stack-v0 envs on one GPU (drop-in for `ParallelEnv`, utils.py:302)."""

  def __init__(self, n_parallel=None, block=None, seed=None, pool=None, device=None,
               env_index_offset=0, side_stream=False, concurrent_envs=None, stream_priority=None, launch_order=None,
               **kwargs):
    """
    Args:
      n_parallel: number of environments B (utils.py:324).
      block: whether step/reset block by default; None -> False (utils.py:326-327).
      seed: env i uses (seed + env_index_offset + i) % 2**32 (utils.py:433).
      pool: `assets.MeshPool` (the urdf list of env.py:92-103); None -> synthetic default pool.
      device: torch device (defaults to the current cuda device).
      env_index_offset: global index of env 0 when the batch is sharded over ranks.
      side_stream: run the env kernels on their own HIP stream so that a non-blocking `step` overlaps the
        caller's work on the current stream (the reference overlaps env processes with `agent.train()`,
        training.py:359-368); the returned callable joins the streams.
      stream_priority: priority of the side stream (-1 = high: the dispatcher serves the env's long-running workgroups
        before the kernels of the current stream; None / 0 = default).
      concurrent_envs: envs that step on the device at the same time over all handles of the caller (a tuning hint for
        the settle kernel's build, `srl_set_concurrent_envs`; results do not depend on it).  None -> this handle alone.
      launch_order: order in which the settle kernel's workgroups take the envs (`srl_set_launch_order`): None -> by batch
        size, False -> index order, True -> the envs with the highest release first.  Results do not depend on it.
      kwargs: StackEnv arguments (env.py:28-51), e.g. episode_length, sim_time_step, rewarder.
    """
    if not torch.cuda.is_available():
      raise RuntimeError('VecStackEnv needs a HIP device: there is no CPU fallback in the product path.')
    self._lib = _lib.load()
    self._device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    self.config = StackConfig(n_envs=int(n_parallel or 1), env_index_offset=int(env_index_offset), **kwargs)
    self._block = block
    self._c = self.config.to_c()
    self._h = ctypes.c_void_p()
    with torch.cuda.device(self._device):
      _check(self._lib.srl_create(ctypes.byref(self._c), ctypes.byref(self._h)))
      if concurrent_envs:
        _check(self._lib.srl_set_concurrent_envs(self._h, int(concurrent_envs)))
      if launch_order is not None:
        _check(self._lib.srl_set_launch_order(self._h, int(bool(launch_order))))
      self.pool = pool if pool is not None else _assets.default_pool()
      p = self.pool
      _check(self._lib.srl_load_meshes(self._h, _np_ptr(p.verts), _np_ptr(p.vert_off), _np_ptr(p.tris),
                                       _np_ptr(p.tri_off), _np_ptr(p.mass_com), len(p)))
    B, H, h = self.config.n_envs, self.config.overhead_res, self.config.object_res
    # TestStackEnv (env.py:443-470): one object map per observable orientation, action = orientation * A + pixel
    self._no = self.config.n_object_maps   # with ordering freedom: the maps of every rock of the episode (empty once placed)
    dt = TORCH_DTYPES[self.config.dtype]   # both tensors, env.py:182-205
    self._observation_spec = (TensorSpec((H, H, 2), dt),
                              TensorSpec((h, h, 1) if self._no == 1 else (self._no, h, h, 1), dt))
    self._action_spec = TensorSpec((), torch.int64)
    self._B, self._H, self._hh = B, H, h
    self._closed = False
    self._left = 0          # rocks of the running episode not yet placed (host mirror of the lock-step episode machine)
    self._last = None       # the latest step's ((obs_map, obs_obj), reward, done): what `get_state` stores
    self._needs_reset = False     # `set_pool` has replaced the mesh table under the running episode
    self._script_pending = False  # `set_script` has named mesh ids for the next reset
    self._holds_at_reset = False  # an auto-reset call may hold some envs (`StartedVecStackEnv` with random lengths): their script stays
    self._side = torch.cuda.Stream(device=self._device, priority=int(stream_priority or 0)) if side_stream else None
    self.seed(seed if seed is not None else 0)

  # ---- properties (utils.py:270-281, :417-422)
  @property
  def multiprocessing(self):
    return False

  @property
  def batch_size(self):
    return self._B

  @property
  def observation_spec(self):
    return self._observation_spec

  @property
  def action_spec(self):
    return self._action_spec

  @property
  def n_actions(self):
    return self.config.n_actions * self._no

  @property
  def num_maps_on_show(self):
    """Object maps that hold a rock in the latest observation (`Observer.num_objects`, observer.py:370-376, as
    env.py:596-608 uses it to size the spaces): an action's index must be below this.  Every env of the batch is at
    the same point of its episode, so this is one number (valid once the latest step has been waited for)."""
    if self.config.ordering_freedom:
      return self._left * self.config.n_orientations
    return self.config.n_orientations if self._left > 0 else 0

  def __call__(self, *args, **kwargs):
    return self.step(*args, **kwargs)

  def __del__(self):
    try:
      self.terminate()
    except Exception:
      pass

  # ---- lifecycle
  def terminate(self):
    if getattr(self, '_h', None) and not self._closed:
      self._closed = True
      self._lib.srl_destroy(self._h)
      self._h = None

  def close(self):
    self.terminate()

  def seed(self, seed):
    """utils.py:522-532: returns the list of per-env seeds."""
    seed = int(seed) % 2**32
    _check(self._lib.srl_seed(self._h, seed))
    off = self.config.env_index_offset
    return [[(seed + off + i) % 2**32] for i in range(self._B)]

  def set_script(self, mesh_ids, goal_rect):
    """Explicit episode script for the next reset (parity harness)."""
    mesh_ids = np.ascontiguousarray(mesh_ids, np.int32)
    goal_rect = np.ascontiguousarray(goal_rect, np.int32)
    if mesh_ids.shape != (self._B, self.config.episode_length) or goal_rect.shape != (self._B, 4):
      raise ValueError('script shapes must be [B, L] and [B, 4]')
    _check(self._lib.srl_set_script(self._h, _np_ptr(mesh_ids), _np_ptr(goal_rect)))
    self._script_pending = True

  def set_pool(self, pool):
    """Load another `assets.MeshPool` into the live env (`srl_load_meshes` once more; it waits for the device): the
    rocks of the next episodes come from it, e.g. a pool `rocks.generate_pool` has just made.  The bodies of the running
    episode belong to the old mesh table, so `step` (and `render`, `step_simulation`) is refused until the next `reset`.
    An episode script waiting for the next reset names meshes of the old table: `set_pool` refuses then (set the script
    after it).  The state signature changes with the mesh table: states taken before are refused, a whole-batch `set_state` of
    a state of the new table (a sibling env's) stands for the reset, and a `Lookahead` on this env reloads its scratch env
    at its next `evaluate`."""
    if len(pool) < 1:
      raise AssertionError('List of object descriptor files is empty.')       # env.py:103
    if self._script_pending:
      raise RuntimeError('an episode script is waiting for the next reset: call set_script after set_pool')
    with torch.cuda.device(self._device):
      torch.cuda.synchronize(self._device)
      _check(self._lib.srl_load_meshes(self._h, _np_ptr(pool.verts), _np_ptr(pool.vert_off), _np_ptr(pool.tris),
                                       _np_ptr(pool.tri_off), _np_ptr(pool.mass_com), len(pool)))
    self.pool = pool
    self._left = 0
    self._last = None
    self._needs_reset = True

  def _require_reset(self, what):
    if self._needs_reset:
      raise RuntimeError('{} after set_pool needs a reset first: the running episode belongs to the old pool'.format(what))

  # ---- stepping
  def _stream(self):
    st = self._side if self._side is not None else torch.cuda.current_stream(self._device)
    return ctypes.c_void_p(st.cuda_stream)

  def _fork(self):
    if self._side is not None:      # env kernels start after everything already queued by the caller (the action)
      self._side.wait_stream(torch.cuda.current_stream(self._device))

  def _join(self):
    if self._side is not None:
      torch.cuda.current_stream(self._device).wait_stream(self._side)

  def _launch(self, export, *args, tensors=(), join=True):
    """`export(handle, *args, stream)` on the env's stream: after what the caller has queued (`_fork`), on the env's device, with
    `tensors` (None entries skipped) kept from the caching allocator while the side stream uses them; then the caller's stream
    waits for it, unless a `wait` returned later does (`join=False`)."""
    self._fork()
    with torch.cuda.device(self._device):
      _check(getattr(self._lib, export)(self._h, *args, self._stream()))
    if self._side is not None:
      for t in tensors:
        if t is not None:
          t.record_stream(self._side)
    if join:
      self._join()

  def _new_obs(self):
    dt = self._observation_spec[0].dtype
    return (torch.empty((self._B, self._H, self._H, 2), dtype=dt, device=self._device),
            torch.empty((self._B,) + tuple(self._observation_spec[1].shape), dtype=dt, device=self._device))

  def _finish(self, out):
    def wait():
      _check(self._lib.srl_sync_status(self._h, self._stream()))
      self._join()
      return out
    return wait

  def reset(self, block=None, out=None):
    """out: optional (obs_map, obs_obj) tensors to write into (views of a larger batch, `PipelinedVecStackEnv`)."""
    om, oo = self._new_obs() if out is None else out
    self._launch('srl_reset', om.data_ptr(), oo.data_ptr(), tensors=(om, oo), join=False)
    self._left = self.config.episode_length
    self._needs_reset = self._script_pending = False
    keys = self.config.reward_keys
    out = ((om, oo), torch.zeros(self._B if keys is None else (self._B, len(keys)), dtype=torch.float32, device=self._device),
           torch.zeros(self._B, dtype=torch.bool, device=self._device))     # utils.py:545-552
    self._last = out
    wait = self._finish(out)
    block = self._block if block is None else block
    return wait() if block else wait

  def step(self, action, block=None, out=None):
    """out: optional (obs_map, obs_obj, reward, done uint8) tensors to write into (contiguous views of a larger batch)."""
    self._require_reset('step')
    if not torch.is_tensor(action):
      action = torch.as_tensor(action)
    action = action.to(device=self._device, dtype=torch.int64).contiguous()
    if action.shape != (self._B,):
      raise ValueError('action must have shape [{}]'.format(self._B))
    keys = self.config.reward_keys       # 'all' / 'eval': one column per key of the reference's dict (rewarder.py:147-158)
    if out is None:
      om, oo = self._new_obs()
      reward = torch.empty(self._B if keys is None else (self._B, len(keys)), dtype=torch.float32, device=self._device)
      done = torch.empty(self._B, dtype=torch.uint8, device=self._device)
    else:
      om, oo, reward, done = out
    self._launch('srl_step', action.data_ptr(), om.data_ptr(), oo.data_ptr(), reward.data_ptr(), done.data_ptr(),
                 tensors=(om, oo, reward, done, action), join=False)
    if self._left == 0 and not self._holds_at_reset:   # the auto-reset of every env has taken the script, as `reset` does
      self._script_pending = False
    self._left = self.config.episode_length if self._left == 0 else self._left - 1   # env.py:235-236: auto-reset
    out = ((om, oo), reward, done.view(torch.bool))
    self._last = out
    self._keep = action   # keep the action tensor alive until the kernels consumed it
    wait = self._finish(out)
    block = self._block if block is None else block
    return wait() if block else wait

  def sample(self):
    """utils.py:534-538: a batch of uniform random actions."""
    a = torch.empty(self._B, dtype=torch.int64, device=self._device)
    self._launch('srl_sample', a.data_ptr(), tensors=(a,))
    return a

  # ---- states as values (stackrl_amd/state.py; csrc/state.hip)
  def state_signature(self):
    """`srl_state_signature`: what another handle must share with this one to take its records."""
    sig = ctypes.c_uint64()
    _check(self._lib.srl_state_signature(self._h, ctypes.byref(sig)))
    return int(sig.value)

  def _index_tensor(self, idx):
    return None if idx is None else torch.as_tensor(idx, dtype=torch.int32).to(self._device).contiguous()

  def _get_records(self, indexes=None):
    """(records int32 [n, words] of the envs `indexes` (None = all), seed, sample counter), after the latest step on the
    env's stream, with the fork / join of `render`."""
    idx = self._index_tensor(indexes)
    n = self._B if idx is None else int(idx.numel())
    words = _state.layout(self.config)[0]
    rec = torch.empty((n, words), dtype=torch.int32, device=self._device)
    seed, counter = ctypes.c_uint32(), ctypes.c_uint32()
    self._launch('srl_state_get', None if idx is None else idx.data_ptr(), n, rec.data_ptr(), ctypes.byref(seed),
                 ctypes.byref(counter), tensors=(rec, idx))
    return rec, int(seed.value), int(counter.value)

  def _set_records(self, records, signature, dst=None, src=None):
    """Env dst[i] takes record src[i] of `records` (None = i), `srl_state_set`; the indexes have been checked (`plan_set`)."""
    records = records.to(device=self._device, dtype=torch.int32).contiguous()
    d, s = self._index_tensor(dst), self._index_tensor(src)
    n = int(d.numel()) if d is not None else (int(s.numel()) if s is not None else int(records.shape[0]))
    self._launch('srl_state_set', ctypes.c_uint64(int(signature)), None if d is None else d.data_ptr(),
                 None if s is None else s.data_ptr(), n, records.data_ptr(), tensors=(records, d, s))

  def _host_extra(self, idx):
    return {}

  def _set_host_extra(self, extra, dst, src, whole):
    pass

  def get_state(self, indexes=None):
    """The state of the envs `indexes` (None = all) after the latest step, as an `EnvState`: their records, the latest
    step's observation, reward and done, and the host side of the episode machine.  Runs on the env's stream like `render`;
    nothing is waited for.  Randomness belongs to the slot: env i draws from the key seed + env_index_offset + i with the
    episode counter its record holds, so a record put into another slot (`set_state(..., indexes=...)`, `Lookahead`) continues
    bit for bit until that slot's next reset, which draws the slot's own stream."""
    if self._last is None:
      raise RuntimeError('get_state needs a reset first')
    idx = _state._index_list(indexes, 'indexes')
    rec, seed, counter = self._get_records(idx)
    (om, oo), r, d = self._last
    if idx is None:
      obs, r, d = (om.clone(), oo.clone()), r.clone(), d.clone()
    else:
      i = torch.as_tensor(idx, dtype=torch.int64, device=self._device)
      obs, r, d = (om[i], oo[i]), r[i], d[i]
    return _state.EnvState(rec, obs, r, d, self._left, seed, counter, self.state_signature(), self._host_extra(idx))

  def set_state(self, state, indexes=None, source=None):
    """Env indexes[i] takes record source[i] of `state` (None = i; records may repeat, the indexes may not) and the stored
    `((obs_map, obs_obj), reward, done)` of the envs written is returned: the step tuple the env would have returned there.
    With `indexes=None` the whole batch returns to the snapshot, its rocks-left count, seed and sample counter included.  A
    partial set needs the snapshot at the env's own point of the episode (`ValueError` otherwise), and leaves the handle's
    seed and sample counter alone.  `ValueError` too for a state of another configuration, pool or build, and for repeated
    indexes.  The RNG key stays the slot's (see `get_state`)."""
    dst, src, whole = _state.plan_set(state, self.state_signature(), self._left, self._B, indexes, source)
    if not whole and self._last is None:
      raise RuntimeError('a partial set_state needs a reset first')
    state = state.to(self._device)
    self._set_records(state.records, state.signature, dst, src)
    out = state.step_tuple(src)
    if whole:
      _check(self._lib.srl_state_set_rng(self._h, state.seed, state.sample_counter))
      self._left = state.left
      self._last = out
      self._needs_reset = False       # (the signature has been checked: a whole episode of the table now loaded)
    else:
      (om, oo), r, d = self._last
      i = torch.as_tensor(dst, dtype=torch.int64, device=self._device)
      om, oo, r, d = om.clone(), oo.clone(), r.clone(), d.clone()
      om[i], oo[i], r[i], d[i] = out[0][0], out[0][1], out[1], out[2]
      self._last = ((om, oo), r, d)
    self._set_host_extra(state.extra, dst, src, whole)
    return out

  # ---- telemetry (Simulator.poses / n_steps, Observer.state, Rewarder.goal)
  def state(self):
    B = self._B
    poses = np.zeros((B, _config.MAX_BODIES, 8), np.float32)
    nb = np.zeros(B, np.int32)
    sub = np.zeros((B, 2), np.int32)
    st = np.zeros(B, np.int32)
    _check(self._lib.srl_get_state(self._h, _np_ptr(poses), _np_ptr(nb), _np_ptr(sub), _np_ptr(st)))
    return poses, nb, sub, st

  def step_variant(self):
    """Test hook (`srl_get_step_variant`): (threads per env workgroup, pair points per thread, kernel) of the settle kernel
    this handle launches; kernel 0 = srl_k_step, 1 = srl_k_step_pp1, 2 = srl_k_step_pp2, 3 = srl_k_step_t128."""
    t, pp, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _check(self._lib.srl_get_step_variant(self._h, ctypes.byref(t), ctypes.byref(pp), ctypes.byref(k)))
    return t.value, pp.value, k.value

  def velocities(self):
    v = np.zeros((self._B, _config.MAX_BODIES, 8), np.float32)
    _check(self._lib.srl_get_velocities(self._h, _np_ptr(v)))
    return v

  def set_body_state(self, poses=None, velocities=None):
    """`resetBasePositionAndOrientation` / `resetBaseVelocity` (simulator.py:313, :214) for every placed body, in the
    layouts of `state()[0]` / `velocities()`.  Test hook of the closed-form physics cases."""
    p = None if poses is None else np.ascontiguousarray(poses, np.float32)
    v = None if velocities is None else np.ascontiguousarray(velocities, np.float32)
    for a in (p, v):
      if a is not None and a.shape != (self._B, _config.MAX_BODIES, 8):
        raise ValueError('expected an array of shape ({}, {}, 8)'.format(self._B, _config.MAX_BODIES))
    _check(self._lib.srl_set_body_state(self._h, None if p is None else _np_ptr(p), None if v is None else _np_ptr(v)))

  def step_simulation(self, n=1):
    """`pb.stepSimulation` x n on every env (no placement, no stop criterion, no render)."""
    self._require_reset('step_simulation')
    self._launch('srl_step_simulation', int(n))
    _check(self._lib.srl_sync_status(self._h, self._stream()))

  def sweeps(self):
    """Solver sweeps run by the last step of each env (telemetry)."""
    sw = np.zeros(self._B, np.int32)
    _check(self._lib.srl_get_sweeps(self._h, _np_ptr(sw)))
    return sw

  def contacts(self):
    mp = np.zeros(self._B, np.float32)
    npts = np.zeros(self._B, np.int32)
    _check(self._lib.srl_get_contacts(self._h, _np_ptr(mp), _np_ptr(npts)))
    return mp, npts

  def contact_max_points(self):
    """`srl_contact_max_points`: the most contacts an env can hold (every ground manifold and every manifold slot full)."""
    n = ctypes.c_int32()
    _check(self._lib.srl_contact_max_points(self._h, ctypes.byref(n)))
    return int(n.value)

  def contact_points(self, last=False, capacity=None, wrench=False, out=None):
    """The contact points of every env's pile after the latest step, gathered on the device (`srl_contact_points`;
    include/stackrl_hip.h holds the definition): a `stackrl_amd.contacts.ContactPoints` of device tensors.
      last      only the contacts of the last placed rock: the reference's `Simulator.contact_points` (simulator.py:131-133)
      capacity  rows per env; None = `contact_max_points()`, which no env exceeds.  `count` is the true number either way
      wrench    also the net contact force and torque on every body, [B, episode_length, 8]; it covers all contacts
      out       a `ContactPoints` to fill in place of new tensors (its row count is the capacity); rows at or beyond an env's
                count are left as they were
    Runs on the env's stream like `render`: nothing is waited for, the env is only read."""
    from stackrl_amd import contacts as _contacts
    L = self.config.episode_length
    if out is None:
      C = self.contact_max_points() if capacity is None else int(capacity)
      out = _contacts.empty(self._B, max(C, 0), L, wrench, self._device)   # (a capacity < 1: the export refuses, in its own words)
    else:
      C = _contacts.check_out(out, self._B, L, wrench, self._device)
      if capacity is not None and int(capacity) != C:
        raise ValueError('capacity {} is not the row count of out ({})'.format(capacity, C))
    w = out.wrench if wrench else None
    self._launch('srl_contact_points', int(last), C, out.count.data_ptr(),
                 out.bodies.data_ptr(), out.rows.data_ptr(), None if w is None else w.data_ptr(),
                 tensors=(out.count, out.bodies, out.rows, w))
    return out if wrench or out.wrench is None else _contacts.ContactPoints(out.count, out.bodies, out.rows, None)

  # ---- push test (stackrl_amd/push.py; csrc/push.hip)
  def poses(self, out=None):
    """`Simulator.poses` of every env on the device (`srl_poses`): (poses float32 [B, L, 8], n_bodies int32 [B]) with L =
    episode_length — per body slot x y z qx qy qz qw and the mesh id as the bits of an int32 (`poses[..., 7].view(torch.int32)`),
    zero rows at or above the env's body count.  out: (poses, n_bodies) tensors to fill.  Runs on the env's stream like
    `render`: nothing is waited for, the env is only read."""
    from stackrl_amd import push as _push
    L = self.config.episode_length
    if out is None:
      out = (torch.empty((self._B, L, 8), dtype=torch.float32, device=self._device), torch.empty(self._B, dtype=torch.int32, device=self._device))
    poses, nb = out
    _push.check_tensors('out', [(poses, (self._B, L, 8), torch.float32), (nb, (self._B,), torch.int32)], self._device)
    self._launch('srl_poses', poses.data_ptr(), nb.data_ptr(), tensors=(poses, nb))
    return poses, nb

  def kick(self, dv, select='all'):
    """Adds the velocity increment `dv` to the placed rocks on the device (`srl_kick`): [B, 8] or [B, 3], one increment per
    env, or [B, L, 8] or [B, L, 3], one per body slot; columns 0 - 2 are linear (m/s), 4 - 6 angular (rad/s), the 3-column forms
    linear only.  select: 'all' rocks, the 'last' placed one, or a body slot (a slot the env has not filled is left alone).
    Nothing is waited for.  Like `set_body_state` it leaves the staged records stale: `get_state` is refused until the next
    step."""
    from stackrl_amd import push as _push
    self._require_reset('kick')
    dv, per_body = _push.increments(dv, self._B, self.config.episode_length, self._device)
    self._launch('srl_kick', dv.data_ptr(), per_body, _push.select_code(select), tensors=(dv,))

  def distances(self, since=None, tol=None, out=None):
    """How far every rock is from a reference pose, measured on the device (`srl_pose_distances`): a
    `stackrl_amd.push.PoseDistances`.  since=None measures from the pose each rock was placed at — the reference's
    `Simulator.distances_from_place`, what the discounted rewards use; since=(poses, n_bodies) as `poses()` returned them
    earlier measures from there (a rock placed since: from its place pose; n_bodies None: every row counts) — `Simulator.distances`
    of the steps between.
    tol = (metres, radians) beyond which a rock counts as `moved` (None: `push.default_tol`).  out: a `PoseDistances` to
    fill.  Nothing is waited for, the env is only read."""
    from stackrl_amd import push as _push
    L = self.config.episode_length
    tp, to = _push.default_tol(self.config) if tol is None else tol
    if out is None:
      out = _push.empty(self._B, L, self._device, self.config.velocity_threshold)
    _push.check_tensors('out', [(out.rows, (self._B, L, _push.ROW_WORDS), torch.float32),
                                (out.summary, (self._B, _push.SUMMARY_WORDS), torch.float32)], self._device)
    ref, ref_nb = (None, None) if since is None else since
    if since is not None:      # (n_bodies may be None: every row of the poses counts)
      _push.check_tensors('since', [(ref, (self._B, L, 8), torch.float32)] + ([] if ref_nb is None else [(ref_nb, (self._B,), torch.int32)]),
                          self._device)
    self._launch('srl_pose_distances', None if ref is None else ref.data_ptr(), None if ref_nb is None else ref_nb.data_ptr(),
                 float(tp), float(to), out.rows.data_ptr(), out.summary.data_ptr(), tensors=(ref, ref_nb, out.rows, out.summary))
    return out

  def push(self, dv, substeps, select='all', tol=None):
    """A push test IN PLACE: `poses()`, `kick(dv, select)`, `step_simulation(substeps)`, then `distances(since=...)` from the
    poses before the kick.  The env's own piles are pushed (use `push.PushTest` for a fork): until the next step the latest
    observation no longer shows them and the staged records are stale, so `get_state` is refused; the next step renders the
    piles as the push left them.  Waits for the sub-steps as `step_simulation` does."""
    before = self.poses()
    self.kick(dv, select)
    self.step_simulation(substeps)
    return self.distances(since=before, tol=tol)

  def maps(self):
    Hm = np.zeros((self._B, self._H, self._H), np.float32)
    Om = np.zeros((self._B, self._hh, self._hh) if self._no == 1 else (self._B, self._no, self._hh, self._hh), np.float32)
    g = np.zeros((self._B, 4), np.int32)
    _check(self._lib.srl_get_maps(self._h, _np_ptr(Hm), _np_ptr(Om), _np_ptr(g)))
    return Hm, Om, g

  def object_map(self, mesh_id):
    k = self.config.n_orientations
    o = np.zeros((self._hh, self._hh) if k == 1 else (k, self._hh, self._hh), np.float32)
    _check(self._lib.srl_get_object_map(self._h, int(mesh_id), _np_ptr(o)))
    return o

  def render_heightmap(self, poses, mesh_ids, n_bodies, out=None):
    """O1 on explicit poses: poses f32[B,32,7], mesh_ids i32[B,32], n_bodies i32[B] (device tensors)."""
    if out is None:
      out = torch.empty((self._B, self._H, self._H), dtype=torch.float32, device=self._device)
    self._launch('srl_render_heightmap', poses.data_ptr(), mesh_ids.data_ptr(), n_bodies.data_ptr(), out.data_ptr(),
                 tensors=(poses, mesh_ids, n_bodies, out))
    return out

  def render(self, mode='rgb_array', dtype=None, out=None):
    """`StackEnv.render(mode='rgb_array')` (env.py:295-332; `TestStackEnv.render`, :558-596) of every env:
    (rgb0 [B, H, H, 3], rgb1 [B, h, h, 3]) device tensors — the overhead map coloured by elevation with the goal rectangle
    marked in the green channel, and the object map on show (orientation 0 of the pending rock; with ordering freedom of
    the first rock still unplaced).  float64 like the reference's by default; dtype='uint8' gives frames.  The images are
    those of the latest step, whether or not it has been waited for.  out: optional (rgb0, rgb1) tensors to write into."""
    if mode != 'rgb_array':
      raise ValueError("Invalid value {} for argument mode. Only 'rgb_array' is supported.".format(mode))
    code, dt = _view_dtype(dtype)
    if code < 0:     # the export refuses it, in its own words
      _check(self._lib.srl_render_rgb(self._h, code, None, None, None))
    self._require_reset('render')
    shapes = ((self._B, self._H, self._H, 3), (self._B, self._hh, self._hh, 3))
    if out is None:
      out = tuple(torch.empty(s, dtype=dt, device=self._device) for s in shapes)
    rgb0, rgb1 = out
    for t, s in zip((rgb0, rgb1), shapes):
      if tuple(t.shape) != s or t.dtype != dt or t.device != self._device or not t.is_contiguous():
        raise ValueError('out must be contiguous {} tensors of shapes {} and {} on {}'.format(dt, shapes[0], shapes[1], self._device))
    self._launch('srl_render_rgb', code, rgb0.data_ptr(), rgb1.data_ptr(), tensors=(rgb0, rgb1))
    return rgb0, rgb1

  def _camera_call(self, c, scene, rgb, depth, ids):
    """`srl_render_camera` with the struct `c` on the env's stream, with the fork / join of `render`; any tensor may be None."""
    tensors = tuple(scene or (None,) * 4) + (rgb, depth, ids)
    self._launch('srl_render_camera', ctypes.byref(c), *[None if t is None else t.data_ptr() for t in tensors], tensors=tensors)

  def render_camera(self, width=320, height=240, camera=None, rgb=True, depth=False, ids=False, out=None, scene=None):
    """A perspective view of every env's pile, ray cast on the device (`srl_render_camera`, include/stackrl_hip.h holds the
    definition): the rocks on the grey ground, the observable square in white, the goal rectangle in green, shadows — what
    the reference's `StackEnv(gui=True)` shows in its viewer.  A method of its own: `render` keeps the reference's modes.
      camera  a `stackrl_amd.camera.Camera`; None = `Camera.reference(config)`, the reference's GUI view
      rgb, depth, ids  which images to return, in this order (one tensor when one is asked for, else a tuple):
              uint8 [B, height, width, 3]; float32 [B, height, width], the depth along the viewing direction, +inf for sky;
              int32 [B, height, width], the body slot, -1 ground, -2 sky
      out     tensors to fill in place of new ones: one per image asked for, in that order (views of a larger batch are fine)
      scene   (poses float32 [B, 32, 7], mesh_ids int32 [B, 32], n_bodies int32 [B], goal_rect int32 [B, 4]) to draw instead
              of the env's own state, arrays or device tensors (the layouts of `render_heightmap` plus the goal rectangles)
    The images are those of the latest step, whether or not it has been waited for; the env is only read."""
    from stackrl_amd import camera as _camera
    self._require_reset('render_camera')
    c = (camera if camera is not None else _camera.Camera.reference(self.config)).to_c(width, height)
    want = (bool(rgb), bool(depth), bool(ids))
    specs = [((self._B, c.height, c.width, 3), torch.uint8), ((self._B, c.height, c.width), torch.float32),
             ((self._B, c.height, c.width), torch.int32)]
    if out is not None:
      out = list(out) if isinstance(out, (tuple, list)) else [out]
      if len(out) != sum(want):
        raise ValueError('out must hold one tensor per image asked for ({})'.format(sum(want)))
    ok_size = 1 <= c.width <= 1024 and 1 <= c.height <= 1024     # (otherwise the export refuses, in its own words)
    images = []
    for k, (shape, dt) in enumerate(specs):
      if not want[k]:
        images.append(None)
      elif out is not None:
        t = out.pop(0)
        if tuple(t.shape) != shape or t.dtype != dt or t.device != self._device or not t.is_contiguous():
          raise ValueError('out must be contiguous tensors on {}: {} {}'.format(self._device, dt, shape))
        images.append(t)
      else:
        images.append(torch.empty(shape if ok_size else (0,), dtype=dt, device=self._device))
    if scene is not None:
      shapes = ((self._B, _config.MAX_BODIES, 7), (self._B, _config.MAX_BODIES), (self._B,), (self._B, 4))
      dts = (torch.float32, torch.int32, torch.int32, torch.int32)
      if len(scene) != 4:
        raise ValueError('scene must be (poses, mesh_ids, n_bodies, goal_rect)')
      scene = tuple(torch.as_tensor(a).to(device=self._device, dtype=dt).contiguous() for a, dt in zip(scene, dts))
      for t, sh in zip(scene, shapes):
        if tuple(t.shape) != sh:
          raise ValueError('scene must have shapes {}'.format(shapes))
    self._camera_call(c, scene, *images)
    got = tuple(t for t in images if t is not None)
    return got[0] if len(got) == 1 else got

  def set_profiling(self, enable=True):
    _check(self._lib.srl_set_profiling(self._h, int(bool(enable))))

  def stage_records(self):
    """Test hook (`srl_get_stage_records`): int32 view [B, L, stride, 4] of the rocks' staged render records."""
    stride = int(self._lib.srl_stage_record_stride())
    out = np.zeros((self._B, self.config.episode_length, stride, 4), np.float32)
    _check(self._lib.srl_get_stage_records(self._h, _np_ptr(out), out.size))
    return out

  def kernel_times(self):
    ms = np.zeros(3, np.float32)
    n = np.zeros(3, np.int32)
    _check(self._lib.srl_get_kernel_times(self._h, _np_ptr(ms), _np_ptr(n)))
    return ms, n

  def order_kernel_times(self):
    """(milliseconds, launches) of the ordered launch's two kernels since the last call; call `kernel_times` first."""
    ms = np.zeros(1, np.float32)
    n = np.zeros(1, np.int32)
    _check(self._lib.srl_get_order_kernel_times(self._h, _np_ptr(ms), _np_ptr(n)))
    return float(ms[0]), int(n[0])

  def launch_order(self):
    """Test hook (`srl_get_launch_order`): (keys uint64 [B], order int32 [B]) of the latest ordered launch."""
    keys = np.zeros(self._B, np.uint64)
    order = np.zeros(self._B, np.int32)
    _check(self._lib.srl_get_launch_order(self._h, _np_ptr(keys), _np_ptr(order)))
    return keys, order


class PipelinedVecStackEnv(object):
  """The same B envs as `VecStackEnv(n_parallel=B)` — same seeds, same trajectories, bit for bit — held as `groups`
  handles of B / groups envs, each on its own HIP stream, so that the training loop can treat the groups the way the
  reference's `ParallelEnv` treats its worker processes (utils.py:468-486: every worker is sent its action and answers
  when it is done): `collect_step` evaluates the policy on group k as soon as group k's step has finished and starts
  group k's next step as soon as its actions exist, while the other groups are still settling.

  Why it pays on MI355X: a settle launch lasts as long as its slowest env and for most of
  that time most of its workgroups have finished — at 4,096 envs x 16 rocks about half of the launch's slot-time is
  idle — but the Q-net forward of the NEXT step cannot use those CUs because it needs the observations of every env.
  With two groups the forward of one group runs under the straggler tail of the other.  (More than two groups lose
  again: concurrent settle launches share the CUs round robin, so they all finish late, and HIP multiplexes streams
  over four hardware queues.)

  The plain `ParallelEnv` surface (`reset`, `step`, `sample`, `seed`, ...) is here too; outputs are full-batch tensors
  the groups write their slices of (no copies)."""

  def __init__(self, n_parallel=None, groups=2, block=None, seed=None, pool=None, device=None, env_index_offset=0,
               **kwargs):
    # groups: a count (equal groups; two is the measured optimum, unequal splits of 4,096 envs lose 3 - 6 %) or the sizes
    B = int(n_parallel or 1)
    if isinstance(groups, (tuple, list)):          # explicit group sizes
      sizes = [int(g) for g in groups]
      if any(g < 1 for g in sizes) or sum(sizes) != B:
        raise ValueError('group sizes must be positive and add up to n_parallel')
    else:
      K = int(groups)
      if K < 1 or B % K:
        raise ValueError('n_parallel must be a multiple of groups')
      sizes = [B // K] * K
    K = len(sizes)
    kwargs.pop('side_stream', None)
    kwargs.setdefault('concurrent_envs', B)
    self._block = block
    self._B, self._K = B, K
    self._start = [sum(sizes[:k]) for k in range(K + 1)]
    self.pool = pool if pool is not None else _assets.default_pool()
    self._envs = [VecStackEnv(n_parallel=sizes[k], block=False, seed=seed, pool=self.pool, device=device,
                              env_index_offset=int(env_index_offset) + self._start[k], side_stream=True, **kwargs)
                  for k in range(K)]
    e0 = self._envs[0]
    self.config = e0.config
    self._device = e0._device
    self._cur = None        # the latest step: full-batch tensors + the per-group waits not yet taken

  # ---- the ParallelEnv surface (utils.py:270-281, :417-422)
  multiprocessing = False

  @property
  def batch_size(self):
    return self._B

  @property
  def groups(self):
    return self._K

  @property
  def observation_spec(self):
    return self._envs[0].observation_spec

  @property
  def action_spec(self):
    return self._envs[0].action_spec

  @property
  def n_actions(self):
    return self._envs[0].n_actions

  @property
  def num_maps_on_show(self):
    return self._envs[0].num_maps_on_show

  def __call__(self, *args, **kwargs):
    return self.step(*args, **kwargs)

  def seed(self, seed):
    out = []
    for e in self._envs:
      out += e.seed(seed)
    return out

  def set_script(self, mesh_ids, goal_rect):
    for k, e in enumerate(self._envs):
      e.set_script(mesh_ids[self._slice(k)], goal_rect[self._slice(k)])

  def set_pool(self, pool):
    """`VecStackEnv.set_pool` of every group, after the steps in flight."""
    self.drain()
    for e in self._envs:
      e.set_pool(pool)
    self.pool = pool
    self._cur = None

  def close(self):
    for e in self._envs:
      e.close()

  terminate = close

  def sample(self):
    return torch.cat([e.sample() for e in self._envs])

  def sweeps(self):
    return np.concatenate([e.sweeps() for e in self._envs])

  def state(self):
    return tuple(np.concatenate(x) for x in zip(*[e.state() for e in self._envs]))

  def maps(self):
    return tuple(np.concatenate(x) for x in zip(*[e.maps() for e in self._envs]))

  def render(self, mode='rgb_array', dtype=None):
    """`VecStackEnv.render` of the whole batch, in env order: every group writes its slice, after its own latest step."""
    if mode != 'rgb_array':
      raise ValueError("Invalid value {} for argument mode. Only 'rgb_array' is supported.".format(mode))
    e0 = self._envs[0]
    dt = _view_dtype(dtype)[1] or torch.float64     # (a type the export refuses: the first group's call raises)
    rgb0 = torch.empty((self._B, e0._H, e0._H, 3), dtype=dt, device=self._device)
    rgb1 = torch.empty((self._B, e0._hh, e0._hh, 3), dtype=dt, device=self._device)
    for k, e in enumerate(self._envs):
      e.render(dtype=dtype, out=(rgb0[self._slice(k)], rgb1[self._slice(k)]))
    return rgb0, rgb1

  def render_camera(self, width=320, height=240, camera=None, rgb=True, depth=False, ids=False, scene=None):
    """`VecStackEnv.render_camera` of the whole batch, in env order: every group writes its slice, after its own latest step."""
    want = (bool(rgb), bool(depth), bool(ids))
    w, h = int(width), int(height)
    if not (1 <= w <= 1024 and 1 <= h <= 1024) or not any(want):     # the first group's call raises, in the export's words
      return self._envs[0].render_camera(width, height, camera, rgb, depth, ids, scene=None if scene is None else tuple(a[self._slice(0)] for a in scene))
    specs = (((self._B, h, w, 3), torch.uint8), ((self._B, h, w), torch.float32), ((self._B, h, w), torch.int32))
    full = [torch.empty(s, dtype=dt, device=self._device) for (s, dt), on in zip(specs, want) if on]
    for k, e in enumerate(self._envs):
      sl = self._slice(k)
      e.render_camera(width, height, camera, rgb, depth, ids, out=[t[sl] for t in full],
                      scene=None if scene is None else tuple(a[sl] for a in scene))
    return full[0] if len(full) == 1 else tuple(full)

  def contact_points(self, last=False, capacity=None, wrench=False):
    """`VecStackEnv.contact_points` of the whole batch, in env order: every group writes its slice, after its own latest step."""
    from stackrl_amd import contacts as _contacts
    e0 = self._envs[0]
    C = e0.contact_max_points() if capacity is None else int(capacity)
    if C < 1:                                     # the first group's call raises, in the export's words
      return e0.contact_points(last, C, wrench)
    full = _contacts.empty(self._B, C, self.config.episode_length, wrench, self._device)
    for k, e in enumerate(self._envs):
      sl = self._slice(k)
      e.contact_points(last, None, wrench, out=_contacts.ContactPoints(full.count[sl], full.bodies[sl], full.rows[sl],
                                                                       full.wrench[sl] if wrench else None))
    return full

  def poses(self):
    """`VecStackEnv.poses` of the whole batch, in env order: every group writes its slice, after its own latest step."""
    L = self.config.episode_length
    poses = torch.empty((self._B, L, 8), dtype=torch.float32, device=self._device)
    nb = torch.empty(self._B, dtype=torch.int32, device=self._device)
    for k, e in enumerate(self._envs):
      e.poses(out=(poses[self._slice(k)], nb[self._slice(k)]))
    return poses, nb

  def kick(self, dv, select='all'):
    """`VecStackEnv.kick` over the groups, after `drain()`: `dv` holds the whole batch in env order."""
    from stackrl_amd import push as _push
    dv, _ = _push.increments(dv, self._B, self.config.episode_length, self._device)
    self.drain()
    for k, e in enumerate(self._envs):
      e.kick(dv[self._slice(k)], select)

  def distances(self, since=None, tol=None):
    """`VecStackEnv.distances` of the whole batch, in env order: every group writes its slice, after its own latest step."""
    from stackrl_amd import push as _push
    full = _push.empty(self._B, self.config.episode_length, self._device, self.config.velocity_threshold)
    for k, e in enumerate(self._envs):
      sl = self._slice(k)
      e.distances(since=None if since is None else (since[0][sl], since[1][sl]), tol=tol,
                  out=_push.PoseDistances(full.rows[sl], full.summary[sl], full.velocity_threshold))
    return full

  def push(self, dv, substeps, select='all', tol=None):
    """`VecStackEnv.push` of the whole batch, in place, after `drain()`."""
    before = self.poses()
    self.kick(dv, select)
    for e in self._envs:
      e.step_simulation(substeps)
    return self.distances(since=before, tol=tol)

  def state_signature(self):
    return self._envs[0].state_signature()

  def _group_of(self, i):
    for k in range(self._K):
      if self._start[k] <= i < self._start[k + 1]:
        return k
    raise ValueError('indexes must be in [0, {})'.format(self._B))

  def get_state(self, indexes=None):
    """`VecStackEnv.get_state` of the whole batch (or of the envs `indexes`), group by group after `drain()`, in env order."""
    self.drain()
    idx = _state._index_list(indexes, 'indexes')
    if idx is None:
      parts, order = [e.get_state() for e in self._envs], None
    else:
      groups = [self._group_of(i) for i in idx]
      parts, order = [], []
      for k, e in enumerate(self._envs):
        pos = [p for p, g in enumerate(groups) if g == k]
        if pos:
          parts.append(e.get_state([idx[p] - self._start[k] for p in pos]))
          order += pos
      order = torch.argsort(torch.as_tensor(order, dtype=torch.int64, device=self._device))   # concatenated -> asked-for order

    def cat(f):
      t = torch.cat([f(p) for p in parts])
      return t if order is None else t[order]
    p0 = parts[0]
    return _state.EnvState(cat(lambda p: p.records), (cat(lambda p: p.obs[0]), cat(lambda p: p.obs[1])), cat(lambda p: p.reward),
                           cat(lambda p: p.done), self._envs[0]._left, p0.seed, p0.sample_counter, p0.signature)

  def set_state(self, state, indexes=None, source=None):
    """`VecStackEnv.set_state` over the groups, after `drain()`: env indexes[i] of the whole batch takes record source[i]."""
    self.drain()
    e0 = self._envs[0]
    dst, src, whole = _state.plan_set(state, e0.state_signature(), e0._left, self._B, indexes, source)
    state = state.to(self._device)
    if src is None:
      src = list(range(len(state)))
    for k, e in enumerate(self._envs):
      if whole:
        e.set_state(state, source=src[self._slice(k)])
      else:
        pos = [p for p, i in enumerate(dst) if self._group_of(i) == k]
        if pos:
          e.set_state(state, indexes=[dst[p] - self._start[k] for p in pos], source=[src[p] for p in pos])
    o = self._outputs()      # the latest step is now the restored one
    for k, e in enumerate(self._envs):
      s = self._slice(k)
      (om, oo), r, d = e._last
      o['om'][s], o['oo'][s], o['reward'][s], o['done'][s] = om, oo, r, d.view(torch.uint8)
    self._cur = o
    return state.step_tuple(src)

  def set_profiling(self, enable=True):
    for e in self._envs:
      e.set_profiling(enable)

  def kernel_times(self):
    ms, n = zip(*[e.kernel_times() for e in self._envs])
    return np.sum(ms, 0), np.sum(n, 0)

  def _outputs(self):
    e0 = self._envs[0]
    keys = self.config.reward_keys
    dt = e0._observation_spec[0].dtype
    return dict(
      om=torch.empty((self._B,) + tuple(e0._observation_spec[0].shape), dtype=dt, device=self._device),
      oo=torch.empty((self._B,) + tuple(e0._observation_spec[1].shape), dtype=dt, device=self._device),
      reward=torch.empty(self._B if keys is None else (self._B, len(keys)), dtype=torch.float32, device=self._device),
      done=torch.empty(self._B, dtype=torch.uint8, device=self._device), waits=[None] * self._K)

  def _slice(self, k):
    return slice(self._start[k], self._start[k + 1])

  def _step_tuple(self, o, s=slice(None)):
    return (o['om'][s], o['oo'][s]), o['reward'][s], o['done'][s].view(torch.bool)

  def _wait_group(self, o, k):
    w, o['waits'][k] = o['waits'][k], None
    if w is not None:
      w()                     # srl_sync_status of the group's handle + the current stream waits for the group's stream

  def drain(self):
    """Wait for every step still in flight (before a reset, a checkpoint, the end of a run)."""
    if self._cur is not None:
      for k in range(self._K):
        self._wait_group(self._cur, k)

  def _waiter(self, o):
    def wait():
      for k in range(self._K):
        self._wait_group(o, k)
      return self._step_tuple(o)
    return wait

  def reset(self, block=None):
    self.drain()
    o = self._outputs()
    o['reward'].zero_(); o['done'].zero_()                                # utils.py:545-552
    for k, e in enumerate(self._envs):
      s = self._slice(k)
      o['waits'][k] = e.reset(block=False, out=(o['om'][s], o['oo'][s]))
    self._cur = o
    wait = self._waiter(o)
    block = self._block if block is None else block
    return wait() if block else wait

  def step(self, action, block=None):
    if not torch.is_tensor(action):
      action = torch.as_tensor(action)
    action = action.to(device=self._device, dtype=torch.int64).contiguous()
    if action.shape != (self._B,):
      raise ValueError('action must have shape [{}]'.format(self._B))
    self.drain()
    o = self._outputs()
    for k, e in enumerate(self._envs):
      s = self._slice(k)
      o['waits'][k] = e.step(action[s], block=False, out=(o['om'][s], o['oo'][s], o['reward'][s], o['done'][s]))
    self._cur = o
    wait = self._waiter(o)
    block = self._block if block is None else block
    return wait() if block else wait

  def collect_step(self, policy):
    """`action = policy(step); env.step(action)` of the training loop (training.py:352-357), group by group: the policy
    call on group k waits for group k's latest step only, and group k's next step starts as soon as its actions exist.
      policy(k, index_slice, (state_k, reward_k, terminal_k)) -> int64 actions [B / groups] of group k
    Returns `(step, action)` of the whole batch: the step the policy has just acted on (complete: every group has been
    waited for) and the actions now being carried out.  Nothing is returned to wait on — the next `collect_step`,
    `step`, `reset` or `drain` takes the waits."""
    if self._cur is None:
      raise RuntimeError('collect_step needs a reset first')
    cur, nxt = self._cur, self._outputs()
    action = torch.empty(self._B, dtype=torch.int64, device=self._device)
    for k, e in enumerate(self._envs):
      s = self._slice(k)
      self._wait_group(cur, k)
      action[s] = policy(k, s, self._step_tuple(cur, s))
      nxt['waits'][k] = e.step(action[s], block=False, out=(nxt['om'][s], nxt['oo'][s], nxt['reward'][s], nxt['done'][s]))
    self._cur = nxt
    return self._step_tuple(cur), action


class StartedVecStackEnv(VecStackEnv):
  """`StartedStackEnv` (Stack-v1, env.py:348-441): an episode uses `n_objects` rocks, the first `n_objects -
  episode_length` of which are placed by `start_policy` inside `reset`, so the agent sees only the last
  `episode_length` placements.  The default start policy is the reference's: the lowest placement whose footprint
  lies fully inside the goal (env.py:391-417), evaluated by the heuristic kernels (csrc/heuristics.hip).
  The batch runs in lock step (same episode length everywhere), so the auto-reset call of `step` (env.py:235-236)
  performs the start placements for all envs at once.  With `min_episode_length` every episode draws its own number
  of start placements (env.py:384-387), so the envs finish at different calls: the start placements of the envs a
  call has just reset run inside that call while the others are held (`SRL_ACTION_HOLD`); this mode waits for every
  step (it needs the done flags on the host)."""

  def __init__(self, n_parallel=None, episode_length=15, n_objects=30, start_policy=None, min_episode_length=None,
               **kwargs):
    if n_objects < episode_length:
      raise ValueError("n_objects can't be less than episode_length. Got {} objects for {} steps long episodes.".format(
        n_objects, episode_length))                                            # env.py:375-378
    self._random_lengths = bool(min_episode_length and min_episode_length < episode_length)
    self._lower, self._upper = int(n_objects) - int(episode_length), int(n_objects) - int(min_episode_length or 0)
    dtype = kwargs.get('dtype', 'uint8')
    if start_policy is None and dtype != 'uint8' and (self._upper if self._random_lengths else self._lower) > 0:
      # the default start policy runs the heuristic kernels (csrc/heuristics.hip), which read uint8 observations
      raise ValueError('The default start policy needs dtype uint8 observations (got {}): pass start_policy.'.format(dtype))
    super(StartedVecStackEnv, self).__init__(n_parallel=n_parallel, episode_length=n_objects, **kwargs)
    self._n_start_steps = int(n_objects) - int(episode_length)
    self._holds_at_reset = self._random_lengths
    self._done_prev = None
    if start_policy is None:
      from stackrl_amd import baselines
      # lowest position with the object fully inside the goal: `height` values under the goal-overlap mask
      start_policy = baselines.Baseline('height', goal=True, minorder=0, threshold=1.0)
    elif not callable(start_policy):
      raise TypeError('Invalid type {} for argument start_policy. Must be callable.'.format(type(start_policy)))
    self._start_policy = start_policy
    self._since_reset = 0

  @property
  def n_start_steps(self):
    return self._n_start_steps

  def seed(self, seed):
    self._len_rng = np.random.RandomState(int(seed) % 2**32)   # the episode-length draws (env.py:387)
    return super(StartedVecStackEnv, self).seed(seed)

  def _host_extra(self, idx):
    kind, keys, pos, has_gauss, gauss = self._len_rng.get_state()
    extra = {'since_reset': int(self._since_reset), 'len_rng_keys': torch.from_numpy(keys.astype(np.int64)), 'len_rng_pos': int(pos),
             'len_rng_has_gauss': int(has_gauss), 'len_rng_gauss': float(gauss)}
    if self._done_prev is not None:
      extra['done_prev'] = self._done_prev.clone() if idx is None else self._done_prev[torch.as_tensor(idx, dtype=torch.int64, device=self._device)]
    return extra

  def _set_host_extra(self, extra, dst, src, whole):
    prev = extra.get('done_prev')
    if prev is not None:
      prev = prev.to(self._device)
      if src is not None:
        prev = prev[torch.as_tensor(src, dtype=torch.int64, device=self._device)]
      if whole:
        self._done_prev = prev.clone()
      elif self._done_prev is not None:
        self._done_prev[torch.as_tensor(dst, dtype=torch.int64, device=self._device)] = prev
    if whole:      # the batch's own fields: the episode-length generator and the step count since the reset
      self._since_reset = int(extra['since_reset'])
      self._len_rng.set_state(('MT19937', extra['len_rng_keys'].cpu().numpy().astype(np.uint32), int(extra['len_rng_pos']),
                               int(extra['len_rng_has_gauss']), float(extra['len_rng_gauss'])))

  def set_state(self, state, indexes=None, source=None):
    """`VecStackEnv.set_state`, with the step count since the reset, the done flags of the step before and (whole batch only)
    the state of the episode-length generator."""
    if 'since_reset' not in state.extra:
      raise ValueError('the state was not taken from a StartedVecStackEnv')
    if indexes is not None and int(state.extra['since_reset']) != self._since_reset:
      raise ValueError('a partial set_state needs the snapshot at the env\'s own point of the episode')
    return super(StartedVecStackEnv, self).set_state(state, indexes=indexes, source=source)

  def _start_random(self, step, fresh):
    """Start placements of the envs `fresh` (bool [B]) marks as just reset, each with its own count drawn from
    [n_objects - episode_length, n_objects - min_episode_length] (env.py:384-387); the others are held."""
    (om, oo), r, d = step
    counts = torch.from_numpy(self._len_rng.randint(self._lower, self._upper + 1, size=self._B)).to(self._device)
    todo = torch.where(fresh, counts, torch.zeros_like(counts))
    hold = torch.full((self._B,), _config.ACTION_HOLD, dtype=torch.int64, device=self._device)
    for j in range(int(todo.max())):
      a = torch.where(todo > j, self._start_policy((om, oo)).to(torch.int64), hold)
      (om, oo), _, _ = super(StartedVecStackEnv, self).step(a, block=True)   # a held env's observation does not change
    self.last_start_steps = todo
    keep = ~fresh
    return (om, oo), r * keep, d & keep

  def _start(self, step):
    for _ in range(self._n_start_steps):
      step = super(StartedVecStackEnv, self).step(self._start_policy(step[0]), block=True)
    self._since_reset = 0
    return (step[0], torch.zeros_like(step[1]), torch.zeros_like(step[2]))

  def reset(self, block=None):
    out = super(StartedVecStackEnv, self).reset(block=True)
    if self._random_lengths:
      out = self._start_random(out, torch.ones(self._B, dtype=torch.bool, device=self._device))
      self._done_prev = out[2]
    else:
      out = self._start(out)
    self._last = out
    block = self._block if block is None else block
    return out if block else (lambda: out)

  def step(self, action, block=None):
    self._require_reset('step')       # (before the step count moves)
    block = self._block if block is None else block
    if self._random_lengths:
      out = super(StartedVecStackEnv, self).step(action, block=True)
      fresh, self._done_prev = self._done_prev, out[2]
      if bool(fresh.any()):       # this call was the auto-reset of those envs (env.py:235-236)
        out = self._start_random(out, fresh)
      self._last = out
      return out if block else (lambda: out)
    if self._since_reset == self.config.episode_length - self._n_start_steps:
      # every env is done: this call is the auto-reset (env.py:235-236), followed by the start placements
      out = self._start(super(StartedVecStackEnv, self).step(action, block=True))
      self._last = out
      return out if block else (lambda: out)
    self._since_reset += 1
    return super(StartedVecStackEnv, self).step(action, block=block)


# constructor arguments of the reference's entry points, in signature order, with the registry's kwargs applied
# (env.py:28-51, :349-357, :444-449; envs/stack/__init__.py:4-27) — what `make(as_path=True)` names a directory after
_REF_ARGS = (('episode_length', 30), ('urdfs', '[5-9]?'), ('object_max_dimension', 0.125), ('use_gui', False),
             ('simulator', None), ('sim_time_step', 1 / 100.), ('gravity', 9.8), ('num_sim_steps', None),
             ('velocity_threshold', 0.01), ('smooth_placing', True), ('observer', None), ('observable_size_ratio', 4),
             ('resolution_factor', 5), ('max_z', 0.375), ('rewarder', None), ('goal_size_ratio', .25),
             ('reward_scale', 1.), ('reward_params', 2), ('flat_action', True), ('dtype', 'uint8'), ('seed', None))
_REF_ENTRY = {
  'Stack-v0': ('StackEnv', _REF_ARGS),
  # StartedStackEnv / TestStackEnv take their own arguments and pass the rest on as **kwargs, so only those appear
  # in the signature the reference inspects (utils.py:104-108)
  'Stack-v1': ('StartedStackEnv', (('episode_length', 15), ('min_episode_length', None), ('n_objects', 30),
                                   ('start_policy', None), ('flat_action', True), ('kwargs', None),
                                   ('urdfs', '[5-9]?'), ('reward_params', 2), ('dtype', 'uint8'))),
  'Stack-v2': ('TestStackEnv', (('ordering_freedom', False), ('orientation_freedom', 3), ('kwargs', None),
                                ('urdfs', '[5-9]?'), ('reward_params', 2), ('dtype', 'uint8'))),
}


def env_path(env='Stack-v0', **kwargs):
  """`make(as_path=True)` (utils.py:89-127): the directory name that identifies an env configuration — the entry
  point's class name, then one `<short name><value>` item per argument (all but `seed`): a name of several words is
  shortened to the first letter of the first and three letters of the last, a single word to four letters."""
  if env not in _REF_ENTRY:
    raise ValueError('Invalid env {}'.format(env))
  name, args = _REF_ENTRY[env]
  args = dict(args)
  args.update(kwargs)
  items = []
  for k, v in args.items():
    if k == 'seed':
      continue
    k = k.split('_')
    k = k[0][:1] + k[-1][:3] if len(k) > 1 else k[0][:4]
    items.append(k + str(v))
  return os.path.join(name, ','.join(items).replace(' ', '').replace("'", '').replace('"', ''))


def make(env='Stack-v0', n_parallel=None, block=None, seed=None, as_path=False, **kwargs):
  """`stackrl.envs.make` (utils.py:44-141): 'Stack-v0' (envs/stack/__init__.py:4-8), 'Stack-v1' (`StartedStackEnv`,
  env.py:348-441) and 'Stack-v2' (`TestStackEnv`, env.py:443-470, with its default `orientation_freedom=3`;
  `ordering_freedom=True` shows every rock of the episode and lets the action choose the next one)."""
  if as_path:
    return env_path(env, **kwargs)
  urdfs = kwargs.pop('urdfs', None)                      # env.py:92-103: which irregularity families the episode draws from
  if urdfs is not None:
    from stackrl_amd import assets
    kwargs['pool'] = (kwargs.get('pool') or assets.default_pool()).select(urdfs)
  if env == 'Stack-v2':
    kwargs.setdefault('orientation_freedom', 3)
  elif env == 'Stack-v1':
    return StartedVecStackEnv(n_parallel=n_parallel or 1, block=block, seed=seed, **kwargs)
  elif env != 'Stack-v0':
    raise ValueError("Invalid env {}: 'Stack-v0', 'Stack-v1' and 'Stack-v2' are implemented.".format(env))
  groups = kwargs.pop('groups', None)                    # build option: the batch as several handles (PipelinedVecStackEnv)
  if groups and (isinstance(groups, (tuple, list)) or int(groups) > 1):
    return PipelinedVecStackEnv(n_parallel=n_parallel or 1, groups=groups, block=block, seed=seed, **kwargs)
  return VecStackEnv(n_parallel=n_parallel or 1, block=block, seed=seed, **kwargs)


def make_curriculum(env='Stack-v0', n_parallel=None, block=None, curriculum=None, **kwargs):
  """`stackrl.envs.make_curriculum` (utils.py:143-182): a generator of `(env, goal)` tuples.  `curriculum` is a dict of
  equally long lists of `make` keyword arguments (e.g. `urdfs`) plus an optional list `goals` of goal returns."""
  curriculum = dict(curriculum or {})
  goals = curriculum.pop('goals', None)
  stages = [dict(zip(curriculum.keys(), values)) for values in zip(*curriculum.values())]
  if goals is not None and len(goals) != len(stages):
    raise ValueError("length of goals doesn't match number of environments")
  for i, cargs in enumerate(stages):
    instance = make(env, n_parallel=n_parallel, block=block, **cargs, **kwargs)
    yield instance, (None if goals is None else goals[i])
